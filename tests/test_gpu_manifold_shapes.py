"""phamers_amd.manifold past the shapes of tests/test_gpu_manifold.py: neighbour selection with k up to 4096 and hundreds of
ties at the threshold, the perplexity search at its edges, the gradient where a workgroup loops over several column tiles
(and over all of them), PCA across row chunks, ragged widths and past one projection launch, and the control loop of
phk_tsne_fit against the restatement's (tests/manifold_ref.py).

Every tolerance is one of: equality of bits; a figure of tests/golden/manifold.npz (as in test_gpu_manifold.py); a rounding
bound computed from the reference's magnitudes, derived in the test's docstring.  tests/test_manifold_host.py holds the
conditions on the inputs (tie-class sizes, kept rows, decision margins, the one-pass covariance missing the bound)."""
import os
import time

import numpy as np
import pytest

from tests import manifold_ref as ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = np.finfo(np.float64).eps
LD = np.longdouble


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "manifold.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def manifold():
    from phamers_amd import manifold as m
    return m


@pytest.fixture(autouse=True)
def wall_time(request):
    t = time.time()
    yield
    print("[wall] %s: %.1f s" % (request.node.name, time.time() - t))


def tol(fig):
    return max(8.0 * float(fig), 64.0 * EPS)


def close(got, want, fig, what):
    got, want = np.asarray(got), np.asarray(want)
    scale = float(np.max(np.abs(want)))
    err = float(np.max(np.abs(got - want)))
    print("%s: max deviation %.3e of %.3e (allowed %.3e relative)" % (what, err, scale, tol(fig)))
    assert err <= tol(fig) * scale, (what, err / scale, tol(fig))


def same_graph(got, want):
    idx, d2 = got
    assert np.array_equal(idx, want[0])
    assert np.array_equal(d2.view(np.int64), want[1].view(np.int64))


# ---- A. neighbour graph: equality of bits ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n", [(127, 131), (128, 131), (129, 133), (255, 259), (256, 261), (257, 263), (1023, 1027),
                                 (1024, 1029), (1025, 1031), (4095, 4099), (4096, 4101), (4096, 4097)])
def test_neighbours_at_the_edges_of_the_sort_width(manifold, k, n):
    assert n % 64 != 0 and k < n
    Z = ref.synthetic(k, n, 2 + k % 2)
    same_graph(manifold.neighbors(Z, k), ref.neighbors(Z, k))


def test_more_neighbours_than_the_sort_holds_are_refused(manifold):
    X = ref.synthetic(3, 4200, 2)
    with pytest.raises(ValueError, match="k=4097 neighbours"):
        manifold.neighbors(X, 4097)
    with pytest.raises(ValueError, match="k=4099 neighbours: must be between 1 and min"):
        manifold.TSNE(perplexity=1366).fit_transform(X)


@pytest.mark.parametrize("seed,n,side,d,k", ref.LATTICE_CASES)
def test_neighbours_on_integer_lattices(manifold, seed, n, side, d, k):
    """Hundreds of equal distances at the threshold, cut inside the class, across scan steps and waves (the host test
    asserts that of these inputs)."""
    Z = ref.lattice_rows(seed, n, side, d)
    same_graph(manifold.neighbors(Z, k), ref.neighbors(Z, k))


def test_neighbours_of_many_copies_of_one_row(manifold):
    rng = np.random.default_rng(5)
    n, m, k = 700, 300, 100
    Z = rng.standard_normal((n, 3))
    copies = np.sort(rng.choice(n, m, replace=False))
    Z[copies] = Z[copies[0]]
    idx, d2 = manifold.neighbors(Z, k)
    same_graph((idx, d2), ref.neighbors(Z, k))
    for i in copies[[0, 1, m // 2, m - 1]]:       # T = 0, nothing below it: the first k other copies, at +0.0
        assert np.array_equal(idx[i], copies[copies != i][:k])
        assert np.array_equal(d2[i].view(np.int64), np.zeros(k, np.int64))
    for n, k in ((600, 200), (600, 599), (257, 256)):
        Z = np.tile(rng.standard_normal((1, 3)), (n, 1))
        idx, d2 = manifold.neighbors(Z, k)
        others = np.arange(n)[None, :].repeat(n, axis=0)
        others = others[others != np.arange(n)[:, None]].reshape(n, n - 1)[:, :k]
        assert np.array_equal(idx, others)
        assert np.array_equal(d2.view(np.int64), np.zeros((n, k), np.int64))
        same_graph((idx, d2), ref.neighbors(Z, k))


@pytest.mark.parametrize("perplexity,n", [(100.0, 1501), (341.0, 1501), (342.0, 1501), (1365.0, 4201)])
def test_wide_neighbourhoods_through_neighbor_affinities(manifold, gold, perplexity, n):
    X = ref.synthetic(int(perplexity), n, 3)
    k = manifold.n_neighbors_for(n, perplexity)
    assert k == int(3 * perplexity + 1)
    a = manifold.neighbor_affinities(X, perplexity)
    idx, d2 = ref.neighbors(X, k)
    assert a.indices.shape == (n, k)
    same_graph((a.indices, a.sqdistances), (idx, d2))
    rows = np.concatenate(([0, 1, 255, 256, n - 3, n - 1], np.random.default_rng(0).integers(0, n, 26)))
    P, beta, margin = ref.binary_search_perplexity(d2[rows], perplexity, margins=True)
    keep = margin >= 1e-9
    assert keep.sum() >= 0.9 * len(rows)
    close(a.conditional[rows][keep], P[keep], gold["cond_dev"], "conditional P")
    close(a.beta[rows][keep], beta[keep], gold["cond_dev"], "beta")
    csr = ref.symmetrize(a.indices, a.conditional)
    got = a.joint()
    assert np.array_equal(got[0], csr[0]) and np.array_equal(got[1], csr[1])
    close(got[2], csr[2], gold["joint_dev"], "joint P")


# ---- B. perplexity search edges -------------------------------------------------------------------------------------------
def test_perplexity_search_on_a_row_of_zeros(manifold):
    for k, perplexity in ((40, 5.0), (301, 100.0), (4096, 1365.0)):
        P, beta = manifold.conditional_affinities(np.zeros((3, k)), perplexity)
        assert np.all(beta == 2.0 ** 100)                    # H = log k > log perplexity at every one of 100 doublings
        assert np.array_equal(P, np.full((3, k), 1.0 / k))   # every exp is exactly 1


@pytest.mark.parametrize("case", range(len(ref.affinity_edge_cases())))
def test_perplexity_search_edges(manifold, gold, case):
    name, d2, perplexity = ref.affinity_edge_cases()[case]
    Pr, br, margin = ref.binary_search_perplexity(d2, perplexity, margins=True)
    keep = margin >= 1e-9         # (rows whose stopping step another exp could move by one are left out: host test, >= 95%)
    assert np.mean(keep) >= 0.95
    P, beta = manifold.conditional_affinities(d2, perplexity)
    close(P[keep], Pr[keep], gold["cond_dev"], "conditional P, " + name)
    close(beta[keep], br[keep], gold["cond_dev"], "beta, " + name)


# ---- C. gradient and objective where a range holds several tiles ---------------------------------------------------------
def boundary_rows(n):
    tiles, G, first = ref.gradient_ranges(n)
    rows = set()
    for g in (0, G // 2, G - 1):
        rows.update((first[g], first[g] + 1, first[g + 1] - 1, first[g + 1] - 2))
    for g in range(1, G, max(1, G // 6)):
        rows.update((first[g] - 1, first[g]))
    rows.update(int(r) for r in np.random.default_rng(0).integers(0, n, 12))
    return tiles, G, np.array(sorted(r for r in rows if 0 <= r < n))


@pytest.mark.parametrize("n,tiles,G", [(11521, 46, 45), (12000, 47, 44), (20000, 79, 26)])
def test_gradient_where_a_range_holds_several_tiles(manifold, gold, n, tiles, G):
    got_tiles, got_G, rows = boundary_rows(n)
    assert (got_tiles, got_G) == (tiles, G) and G < tiles
    X = ref.synthetic(n, n, 5)
    csr = manifold.neighbor_affinities(X, 30.0).joint()
    Y = 20.0 * np.random.default_rng(1).standard_normal((n, 2))
    kl, g = manifold.kl_gradient(Y, csr)
    kl_r, g_r = ref.kl_gradient(Y, csr, rows=rows)
    close([kl], [kl_r], gold["kl_dev"], "KL")
    scale = float(np.max(np.abs(g)))
    err = float(np.max(np.abs(g[rows] - g_r)))
    print("gradient on %d sampled rows: %.3e of %.3e" % (len(rows), err, scale))
    assert err <= tol(gold["grad_dev"]) * scale
    if n == 12000:
        Y5, Y5r = manifold.descend(Y, csr, 5), ref.descend(Y, csr, 5)
        # five updates add up at most five gradients' deviations (the rule of test_gpu_manifold.test_shapes)
        close(Y5, Y5r, 8 * float(gold["grad_dev"]), "five steps")


def test_gradient_over_all_tiles_in_one_range_on_a_lattice(manifold):
    """n = 2^19 + 257: 2050 tiles, one range (every row's sums are ONE chain over all n columns) and 2050 block sums, more
    than the 256 threads of the total's first stride.  The points lie on a 64 x 64 integer grid with seeded multiplicities,
    so Z and the repulsive sums have a closed reference over cells in np.longdouble (ref.kl_gradient_lattice, pinned to the
    pairwise reference by the host test); coincident points (w = 1, d = 0) are part of it.

    Bounds (eps = 2^-52 = 2 u; Higham (3.5): a chain of m additions of terms with relative error <= c_t u is off by at most
    (m - 1 + c_t) u sum|term|, which is <= m eps sum|term| -- c = 1 -- as long as c_t <= m + 1):
      z_i, r_i : chains of m = n terms, so |dz_i| <= n eps z_i and |dr_i| <= n eps sum_j w^2 |y_i - y_j| =: n eps S_i;
      Z        : the sum of the z_i by a 256-leaf tree, a strided chain of ceil(2050 / 256) = 9 and another tree: 25 more
                 additions, |dZ| <= (n + 32) eps Z;
      grad_i   = 4 (a_i - r_i / Z), a_i a chain over the row's <= 3 entries each with ~6 roundings, A_i = sum|p w d|:
                 |dgrad_i| <= 4 eps (16 A_i + (2 n + 40) S_i / Z)     [n S_i / Z for the chain, (n + 32) |r_i| / Z <= ...
                 S_i / Z for Z, the rest for the division and the final subtraction];
      KL       = sum_e p_e (log p_e - log w_e + log Z) with sum p = 1: the error of log Z enters whole, (n + 32) eps, and the
                 terms' own rounding and their summation (a chain of <= 3, a tree, a chain of 9, a tree) at most
                 64 eps sum|term|."""
    n, side = (1 << 19) + 257, 64
    tiles, G, _ = ref.gradient_ranges(n)
    assert (tiles, G) == (2050, 1)
    Y, cells, counts = ref.lattice_embedding(51, n, side)
    csr = ref.ring_csr(n, 52)
    rows = np.concatenate(([0, 1, 255, 256, 257, 65535, 65536, n // 2, n - 258, n - 257, n - 2, n - 1],
                           np.random.default_rng(2).integers(0, n, 20)))
    kl_r, g_r, Z, S, A, kl_abs = ref.kl_gradient_lattice(Y, cells, counts, csr, rows)
    t = time.time()
    kl, g = manifold.kl_gradient(Y, csr)
    print("device: %.2f s" % (time.time() - t))
    kl_bound = float((n + 32) * EPS + 64 * EPS * kl_abs)
    print("KL %.12g: deviation %.3e, bound %.3e" % (kl, abs(kl - float(kl_r)), kl_bound))
    g_bound = (4 * EPS * (16 * A + (2 * n + 40) * S / Z)).astype(np.float64)
    err = np.abs(g[rows].astype(LD) - g_r).astype(np.float64)
    worst = int(np.argmax(err / g_bound)) // 2
    print("gradient: largest deviation %.3e (row %d: bound %.3e, |g| %.3e); largest deviation / bound %.3e"
          % (err.max(), rows[worst], g_bound[worst].max(), np.abs(g_r[worst]).max(), np.max(err / g_bound)))
    assert abs(kl - float(kl_r)) <= kl_bound
    assert np.all(err <= g_bound)
    assert np.all(np.isfinite(g)) and float(np.max(np.abs(g_r))) > 0


# ---- D. PCA ---------------------------------------------------------------------------------------------------------------
def device_covariance(X):
    from phamers_amd import _lib
    X = np.ascontiguousarray(X, dtype=np.float64)
    n, D = X.shape
    mean, cov = np.empty(D), np.empty((D, D))
    ctx = _lib.get_context()
    _lib.check(ctx.lib.phk_pca_covariance(ctx.handle, _lib.ptr(X), n, D, _lib.ptr(mean), _lib.ptr(cov)))
    return mean, cov


@pytest.mark.parametrize("n,D,offset", ref.PCA_CASES)
def test_covariance_across_chunks_and_ragged_widths(manifold, n, D, offset):
    """Mean and covariance against the two-pass np.longdouble reference, under ref.covariance_bound (derived there):
    (rows in the longest chain) eps |Xc|^T |Xc| / (n - 1) elementwise, c = 1; the mean under the same chain length times
    eps times the column's mean magnitude.  For the offset case a one-pass float64 formula misses the bound on this data."""
    X = ref.spectrum_data(n, n, D, offset)
    mean_r, cov_r, gram = ref.covariance(X)
    bound, chain = ref.covariance_bound(n, D, gram)
    mean, cov = device_covariance(X)
    mean_bound = (chain * EPS * np.abs(X).mean(axis=0))
    mean_err = np.abs(mean - mean_r).astype(np.float64)
    err = np.abs(cov - cov_r).astype(np.float64)
    safe = np.where(bound > 0, bound, 1.0)
    print("(%d, %d): chain %d; mean deviation / bound %.3e; covariance deviation %.3e, largest deviation / bound %.3e"
          % (n, D, chain, np.max(mean_err / mean_bound), err.max(), np.max(err / safe)))
    assert np.all(mean_err <= mean_bound)
    assert np.all(err <= bound)
    assert np.array_equal(cov, cov.T) or np.all(np.abs(cov - cov.T) <= 2 * bound)
    if offset:
        one_pass = np.abs(ref.covariance_one_pass(X) - cov_r).astype(np.float64)
        print("one-pass float64 on the same data: largest deviation / bound %.3e" % np.max(one_pass / safe))
        assert np.max(one_pass / safe) > 100.0
    # top components, where the reference's eigenvalue gaps are clear
    c = min(5, n - 1, D - 1)
    w = np.sort(np.linalg.eigvalsh(cov_r.astype(np.float64)))[::-1]
    gaps = (w[:c] - w[1:c + 1]) / w[:c]
    assert np.all(gaps >= 1e-6), gaps
    p = manifold.PCA(c).fit(X)
    Tr, comps, _, var = ref.pca(np.asarray(X, np.float64) - np.asarray(mean_r, np.float64), c)
    assert np.all(p.components_[np.arange(c), np.argmax(np.abs(p.components_), axis=1)] > 0)
    # Davis-Kahan (Yu, Wang & Samworth 2015): |v' - v| <= 2^1.5 |E| / gap, E the difference of the two covariances: the
    # device's bound above in Frobenius norm plus the float64 reference's own, D eps |C|, and as much for each eigh
    E = float(np.linalg.norm(bound)) + 3 * D * EPS * float(w[0])
    abs_gap = np.minimum(w[:c] - w[1:c + 1], np.concatenate(([np.inf], w[:c - 1] - w[1:c])))
    comp_err = np.linalg.norm(p.components_ - comps, axis=1)
    print("components: deviation %s, bound %s" % (comp_err, 2 ** 1.5 * E / abs_gap))
    assert np.all(comp_err <= 2 ** 1.5 * E / abs_gap)
    assert np.all(np.abs(p.explained_variance_ - w[:c]) <= E)


def test_covariance_where_the_cap_sets_the_chunk(manifold):
    """D = 4096: 256 MiB hold two D x D partials, so n = 2101 rows make chunks of 1052 rows (above the floor of 1024), the
    last of 1049 (not a multiple of 4).  The reference is taken on 40 rows of the covariance (all 4096 columns of each)."""
    n, D = ref.PCA_CAP_CASE
    assert ref.pca_chunk_rows(n, D) == 1052
    X = ref.spectrum_data(7, n, D)
    mean, cov = device_covariance(X)
    Xl = X.astype(LD)
    mean_r = Xl.sum(axis=0) / n
    Xc = Xl - mean_r
    pick = np.concatenate(([0, 1, 15, 16, 63, 64, 65, 2047, 2048, D - 2, D - 1], np.random.default_rng(3).integers(0, D, 29)))
    cov_r = Xc[:, pick].T @ Xc / (n - 1)
    bound, chain = ref.covariance_bound(n, D, np.abs(Xc[:, pick]).T @ np.abs(Xc))
    err = np.abs(cov[pick] - cov_r).astype(np.float64)
    print("chain %d: covariance deviation %.3e, largest deviation / bound %.3e" % (chain, err.max(), np.max(err / bound)))
    assert np.all(np.abs(mean - mean_r).astype(np.float64) <= chain * EPS * np.abs(X).mean(axis=0))
    assert np.all(err <= bound)
    assert np.all(np.abs(cov[:, pick].T - cov[pick]) <= 2 * bound)


def test_projection_past_one_launch(manifold):
    """n = 2^21 + 65 rows of D = 2: 32 769 row tiles, the second launch takes the last one.  Every output is a chain of two
    fused multiply-adds of centred values: |error| <= (D + 2) eps sum_d |x_d - mean_d| |v_d| (one rounding per centring,
    one per fma, c = 1 with eps = 2 u)."""
    rng = np.random.default_rng(9)
    n = (1 << 21) + 65
    fit = rng.standard_normal((4000, 2)) * [3.0, 1.0] + [5.0, -2.0]
    p = manifold.PCA(1).fit(fit)
    X = rng.standard_normal((n, 2)) * [3.0, 1.0] + [5.0, -2.0]
    T = p.transform(X)
    assert T.shape == (n, 1)
    Xc = X.astype(LD) - p.mean_.astype(LD)
    want = Xc @ p.components_.astype(LD).T
    bound = (4 * EPS * (np.abs(Xc) @ np.abs(p.components_.astype(LD)).T)).astype(np.float64)
    err = np.abs(T - want).astype(np.float64)
    seam = 32768 * 64
    for name, r in (("first", 0), ("seam - 1", seam - 1), ("seam", seam), ("last", n - 1)):
        print("row %s: %.17g (reference %.17g)" % (name, T[r, 0], float(want[r, 0])))
    print("largest deviation %.3e, largest deviation / bound %.3e" % (err.max(), np.max(err / np.maximum(bound, 1e-300))))
    assert np.all(err <= bound)
    assert np.all(err[[0, seam - 1, seam, seam + 64, n - 1]] <= bound[[0, seam - 1, seam, seam + 64, n - 1]])


# ---- E. the control loop --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ref.CONTROL_CASES))
def test_control_loop(manifold, gold, name):
    """(n_iter_, kl_divergence_) of manifold.TSNE against ref.tsne for every exit of the loop (the host test asserts the
    margin of every decision of these cases).  kl_divergence_: 8 x kl_dev where the embedding has moved through no more
    updates than the fixture's trajectory figure stays rounding-sized for (traj_dev <= 1e-9, the rule of
    test_gpu_manifold.test_trajectory), 1e-3 relative otherwise (the whole-run rule).  No exit of TSNE comes before 100
    updates, so only the case that does not move at all falls under the first.  The embedding is compared where the run is
    no longer than the longest trajectory the fixture records, under that record's figure."""
    X, Y0 = ref.control_problem()
    kw = ref.CONTROL_CASES[name]
    Yr, kl_r, it_r = ref.control_reference(name)
    t = manifold.TSNE(perplexity=ref.CONTROL_PERPLEXITY, init=Y0.copy(), **kw)
    Y = t.fit_transform(X)
    print("%s: n_iter_ %d (reference %d), kl_divergence_ %.12g (reference %.12g)" % (name, t.n_iter_, it_r, t.kl_divergence_, kl_r))
    assert it_r == ref.CONTROL_EXPECTED_N_ITER[name]
    assert t.n_iter_ == it_r
    steps = (it_r + 1 if name != "max_iter_250" else 250) if kw["learning_rate"] > 0 else 0
    vouched = [int(s) for s, d in zip(gold["traj_steps"], gold["traj_dev"]) if d <= 1e-9]
    if kl_r == np.finfo(float).max:
        assert t.kl_divergence_ == kl_r          # the empty second phase: scikit-learn's initial error
    elif steps <= max(vouched):
        close([t.kl_divergence_], [kl_r], gold["kl_dev"], "KL")
    else:
        assert abs(t.kl_divergence_ - kl_r) <= 1e-3 * abs(kl_r)
    if steps == 0:
        assert np.array_equal(Y, Y0)
    elif steps <= int(gold["traj_steps"][-1]):
        dev = float(gold["traj_dev"][[i for i, s in enumerate(gold["traj_steps"]) if s >= steps][0]])
        err, span = float(np.max(np.abs(Y - Yr))), float(np.ptp(Yr))
        print("embedding after %d updates: deviation %.3e of span %.3e (allowed %.3e relative)" % (steps, err, span, 8 * dev))
        assert err <= max(8.0 * dev, 64.0 * EPS) * span
