"""The 64 x 64 pair tile (csrc/pair_tile.h) and the ordered row selection (csrc/row_select.h) through every entry point
that writes the tile out as a matrix, at the smallest shapes where the tile can go wrong: one row, one short of / exactly /
one past a tile side, more than one tile on both sides, one short of / exactly / one past an LDS step of 16 columns and more
than one step.  Everything is held bit for bit to the exact host chain acc = fma(q_c - x_c, q_c - x_c, acc) over the columns
in order (tests.neighbors_ref.sqdist on tests.manifold_ref.fma) and to "the first k in order of (value, index)".  Inputs are
non-dyadic normals of both signs with one duplicated row (a squared distance of +0).  The device's float64 sqrt is taken to
be NumPy's (correctly rounded), as in tests/test_gpu_neighbors.py."""
import numpy as np
import pytest

from tests import manifold_ref, neighbors_ref

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def ctx():
    from phamers_amd import _lib
    return _lib.get_context()


def normals(seed, n, d):
    """n x d normals of both signs, scaled by 1 / 3 (no entry is a short binary fraction)."""
    return np.random.default_rng(seed).standard_normal((n, d)) / 3.0


def same_bits(got, want):
    return got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64))


def distances(ctx, Q, X):
    from phamers_amd import _lib
    Q, X = np.ascontiguousarray(Q), np.ascontiguousarray(X)
    out = np.full((Q.shape[0], X.shape[0]), np.nan)
    _lib.check(ctx.lib.phk_distances(ctx.handle, _lib.ptr(Q), Q.shape[0], _lib.ptr(X), X.shape[0], Q.shape[1], _lib.ptr(out)))
    return out


# ---- phk_distances: query rows and column rows from different matrices, N > 1 ---------------------------------------------
@pytest.mark.parametrize("D", [1, 15, 16, 17, 33])
def test_distances_at_the_edges_of_the_tile(ctx, D):
    Qall, Xall = normals(100 + D, 129, D), normals(200 + D, 130, D)
    Xall[0] = Qall[0]
    for N in (1, 63, 64, 65, 129):
        for M in (1, 64, 65, 130):
            Q, X = Qall[:N], Xall[:M]
            want = np.sqrt(neighbors_ref.sqdist(Q, X))
            got = distances(ctx, Q, X)
            assert same_bits(got, want), (N, M, D, int(np.sum(got != want)))
            assert got[0, 0] == 0.0 and not np.signbit(got[0, 0])


def test_distances_of_a_matrix_to_itself_are_symmetric(ctx):
    X = normals(7, 130, 17)
    X[129] = X[3]
    got = distances(ctx, X, X)
    assert same_bits(got, np.ascontiguousarray(got.T))
    assert same_bits(got, np.sqrt(neighbors_ref.sqdist(X, X)))
    assert np.all(np.diag(got) == 0.0) and got[3, 129] == 0.0


# ---- phk_pca_project: the tile with a product and the column mean taken off the query side ----------------------------------
def project_ref(X, mean, V):
    s = np.zeros((X.shape[0], V.shape[0]))
    for d in range(X.shape[1]):
        s = manifold_ref.fma((X[:, d] - mean[d])[:, None], V[None, :, d], s)
    return s


@pytest.mark.parametrize("D", [1, 16, 17, 70])
def test_projection_at_the_edges_of_the_tile(ctx, D):
    from phamers_amd import _lib
    Xall, mean, Vall = normals(300 + D, 130, D) + 0.7, normals(400 + D, 1, D)[0] + 0.7, normals(500 + D, min(D, 65), D)
    Xall[129] = Xall[0]
    for n in (1, 64, 65, 130):
        for nc in sorted({1, min(D, 2), min(D, 65)}):
            X, V = np.ascontiguousarray(Xall[:n]), np.ascontiguousarray(Vall[:nc])
            out = np.full((n, nc), np.nan)
            _lib.check(ctx.lib.phk_pca_project(ctx.handle, _lib.ptr(X), n, D, _lib.ptr(mean), _lib.ptr(V), nc, _lib.ptr(out)))
            assert same_bits(out, project_ref(X, mean, V)), (n, D, nc)


# ---- phk_tsne_neighbors: the tile with +inf on the diagonal, then the ordered selection --------------------------------------
def tsne_neighbors(ctx, Z, k):
    from phamers_amd import _lib
    Z = np.ascontiguousarray(Z)
    n, d = Z.shape
    idx, d2 = np.full((n, k), -1, np.int32), np.full((n, k), np.nan)
    _lib.check(ctx.lib.phk_tsne_neighbors(ctx.handle, _lib.ptr(Z), n, d, k, _lib.ptr(idx), _lib.ptr(d2)))
    return idx, d2


@pytest.mark.parametrize("kind", ["normals", "lattice"])
@pytest.mark.parametrize("d", [1, 2, 17, 50])
def test_neighbour_graph_at_the_edges_of_the_tile(ctx, kind, d):
    """On the lattice {0, 1, 2}^d (few distinct distances at d <= 2, every row with many equals) the threshold's class is
    cut by the ordered tie scan; on normals by the values."""
    if kind == "normals":
        Zall = normals(600 + d, 130, d)
        Zall[129] = Zall[1]
    else:
        Zall = manifold_ref.lattice_rows(700 + d, 130, 3, d)
    for n in (2, 64, 65, 130):
        Z = Zall[:n]
        for k in sorted({k for k in (1, 2, 3, n - 1) if k <= n - 1}):
            idx, d2 = tsne_neighbors(ctx, Z, k)
            want_idx, want_d2 = manifold_ref.neighbors(Z, k)
            assert np.array_equal(idx, want_idx), (kind, n, d, k)
            assert same_bits(d2, want_d2), (kind, n, d, k)


# ---- the exact scoring path: the tile against the reference rows and against the centroids ---------------------------------
@pytest.mark.parametrize("masked", [False, True])
def test_exact_scores_of_a_small_model(ctx, masked):
    """65 + 66 reference rows, 3 + 2 centroids, D = 16, 3 neighbours, 130 queries through force_exact.
    knn: the majority of the first 3 rows in order of (chain value, index) -- equal bits, and the oracle's votes over the
    rows left in.  kmeans: tanh((e_n - e_p) / (e_p + e_n)) of the square roots of the smallest chain values; subtraction,
    addition, division and sqrt are correctly rounded on both sides, so the two tanh take the same argument and each lies
    within 2 ulp of the true value (the figure both libraries document): 4 eps relative.  combo: the sum of the two, bits."""
    from oracle import oracle
    from phamers_amd import _lib
    D, kn = 16, 3
    pos, neg, Q = normals(1, 65, D), normals(2, 66, D) + 0.1, normals(3, 130, D)
    cpos, cneg = normals(4, 3, D), normals(5, 2, D) + 0.1
    pos[64] = pos[2]
    Q[0] = pos[2]                  # d2 = +0 twice: rows 2 and 64 tie, the lower index first
    Q[1] = cneg[1]
    mask = np.zeros(131, bool)
    if masked:
        mask[[0, 2, 63, 64, 65, 130]] = True
        mask[np.random.default_rng(6).integers(0, 131, 40)] = True
    model = _lib.Model(ctx, pos, neg, cpos, cneg, kn)
    try:
        if masked:
            model.set_column_mask(mask)
        ctx.set_option("force_exact", "1")
        got = {m: model.score(Q, m) for m in ("knn", "kmeans", "combo")}
    finally:
        ctx.set_option("force_exact", "0")
        model.close()
    d2 = neighbors_ref.sqdist(Q, np.vstack((pos, neg)))
    d2[:, mask] = np.inf
    _, idx = neighbors_ref.select(d2, kn)
    votes = (idx < 65).sum(axis=1)
    knn = np.where(2 * votes > kn, 1.0, -1.0)
    assert np.array_equal(got["knn"], knn)
    assert np.array_equal(got["knn"], oracle.knn_score_points(Q, pos[~mask[:65]], neg[~mask[65:]], kn))
    ep = np.sqrt(neighbors_ref.sqdist(Q, cpos).min(axis=1))
    en = np.sqrt(neighbors_ref.sqdist(Q, cneg).min(axis=1))
    kmeans = np.tanh((en - ep) / (ep + en))
    err = np.abs(got["kmeans"] - kmeans)
    print("kmeans: largest deviation %.3e relative (allowed %.3e)" % (np.max(err / np.abs(kmeans)), 4 * EPS))
    assert np.all(err <= 4 * EPS * np.abs(kmeans))
    assert en[1] == 0.0 and ep[1] > 0.0       # (a +0 in the centroid pass: the argument is exactly -1)
    assert same_bits(got["combo"], got["knn"] + got["kmeans"])
