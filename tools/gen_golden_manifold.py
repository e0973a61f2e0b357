"""Writes tests/golden/manifold.npz: scikit-learn's outputs for the stages of phamers_amd.manifold, the measured
restatement-vs-scikit-learn deviations the tests derive their tolerances from, and the finished-embedding yardsticks.
Run on a CPU host with scikit-learn:  python tools/gen_golden_manifold.py

Refuses an input where some row's k-th and (k+1)-th neighbour differ by less than 1e-9 relative (identical distances are
decided by index and are fine): a condition on the inputs, not a measurement."""
import os
import sys

import numpy as np
import scipy
import sklearn
from scipy.sparse import csr_matrix
from sklearn.decomposition import PCA
from sklearn.manifold import TSNE, _t_sne, _utils, trustworthiness
from sklearn.neighbors import NearestNeighbors

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests import manifold_ref as ref   # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
N_STAGE = 300      # rows of each reference matrix for the per-stage fixtures (600 rows)
N_FINAL = 600      # ... for the finished embedding (1 200 rows: the restatement's and six scikit-learn runs fit a sitting)
PERPLEXITY = 30.0


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def reference_tsne_file():
    """What the reference's own scripts/fileIO.py save_tsne_data writes for five points (PHAMERS_REFERENCE = a PhaMers
    checkout)."""
    import tempfile
    root = os.environ.get("PHAMERS_REFERENCE")
    if not root:
        raise SystemExit("set PHAMERS_REFERENCE to a PhaMers checkout: the t-SNE file fixture is written by its scripts/fileIO.py")
    # the module itself is Python 2 (print statements); the function's own text runs as it stands
    with open(os.path.join(root, "scripts", "fileIO.py")) as f:
        src = f.read()
    src = src[src.index("def save_tsne_data("):src.index("def read_tsne_file(")]
    space = {"np": np}
    exec(compile(src, "scripts/fileIO.py:save_tsne_data", "exec"), space)
    pts = np.array([[1.5, -2.25], [1e-5, 123456.789], [0.1, 1.0 / 3.0], [-7.0, 0.0], [2.5e10, -1e-300]])
    ids = np.array(["NC_000001", "contig_2", "3", "phage.4", "b5"])
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "tsne_coordinates.csv")
        space["save_tsne_data"](path, pts, ids, chops=(2, 2, 1))
        with open(path) as f:
            text = f.read()
    return dict(tsne_file_points=pts, tsne_file_ids=ids, tsne_file_text=np.array(text))


def main():
    out = {"versions": np.array([np.__version__, sklearn.__version__, scipy.__version__])}
    out.update(reference_tsne_file())
    for seed, n, d, perp in ref.SHAPE_CASES + [ref.LARGE_CASE]:
        k = min(n - 1, int(3 * perp + 1))
        gap = ref.kth_gap(ref.synthetic(seed, n, d), k)
        assert gap >= 1e-9, ("neighbourhood edge too close", seed, n, d, gap)
    X = ref.reference_rows(GOLDEN, N_STAGE)
    n = X.shape[0]
    # PCA
    sk = PCA(n_components=50, svd_solver="full")
    T = sk.fit_transform(X)
    Tr, comps, mean, var = ref.pca(X, 50)
    out.update(n_stage=N_STAGE, pca_dev_transformed=rel(Tr, T), pca_dev_components=rel(comps, sk.components_),
               pca_dev_mean=rel(mean, sk.mean_), pca_dev_variance=rel(var, sk.explained_variance_))
    Z = Tr
    k = min(n - 1, int(3 * PERPLEXITY + 1))
    assert ref.kth_gap(Z, k) >= 1e-9 and ref.kth_gap(X, k) >= 1e-9
    # neighbours and affinities
    idx, d2 = ref.neighbors(Z, k)
    g = NearestNeighbors(n_neighbors=k).fit(Z).kneighbors_graph(mode="distance")
    g.data **= 2
    g.sort_indices()
    # rows whose neighbourhood edge is a tie between identical distances (duplicate rows) are decided by index here and
    # arbitrarily by scikit-learn: the sets are compared on the other rows, the searches run on this side's graph
    _, d2x = ref.neighbors(Z, k + 1)
    clear = d2x[:, k] > d2x[:, k - 1]
    assert clear.sum() >= 0.9 * n
    assert np.array_equal(np.sort(idx, axis=1)[clear], g.indices.reshape(n, k)[clear]), "neighbour sets differ from scikit-learn's"
    g = csr_matrix((np.take_along_axis(d2, np.argsort(idx, axis=1), axis=1).ravel(), np.sort(idx, axis=1).ravel(),
                    np.arange(0, n * k + 1, k)), shape=(n, n))
    sk_d2 = g.data.reshape(n, k)
    by_col = np.argsort(idx, axis=1)
    P, beta = ref.binary_search_perplexity(d2, PERPLEXITY)
    P_by_col = np.take_along_axis(P, by_col, axis=1)
    cond64 = _utils._binary_search_perplexity(np.take_along_axis(d2, by_col, axis=1).astype(np.float32), PERPLEXITY, 0)
    cond_sk = _utils._binary_search_perplexity(sk_d2.astype(np.float32), PERPLEXITY, 0)
    joint_sk = _t_sne._joint_probabilities_nn(g, PERPLEXITY, 0)
    csr = ref.symmetrize(idx, P)
    Pd = ref.dense(csr)
    out.update(cond_dev_f32=max(rel(P_by_col, cond_sk), rel(P_by_col, cond64)), joint_dev_f32=rel(Pd, joint_sk.toarray()))
    # the same search on identical float64 distances, in float64: the float64-vs-float64 figure of the stage
    # (_binary_search_perplexity only takes float32, so the float64 figure is the restatement run on the float32-rounded
    # distances against it)
    d32 = np.take_along_axis(d2, by_col, axis=1).astype(np.float32).astype(np.float64)
    P32, _ = ref.binary_search_perplexity(d32, PERPLEXITY)
    out.update(cond_dev=rel(P32, cond64))
    j32 = ref.dense(ref.symmetrize(np.sort(idx, axis=1), P32))
    sk32 = csr_matrix((cond64.ravel(), g.indices, g.indptr), shape=(n, n))
    sk32 = sk32 + sk32.T
    sk32 = (sk32 / max(sk32.sum(), ref.MACHINE_EPSILON)).toarray()
    out.update(joint_dev=rel(j32, sk32))
    # objective and gradient at three kinds of Y, against the float64 dense _kl_divergence
    from scipy.spatial.distance import squareform
    Pc = squareform(Pd, checks=False)
    Y_init = Z[:, :2] / np.std(Z[:, 0]) * 1e-4
    Y_mid = ref.descend(Y_init, csr, 60, exaggeration=12.0, momentum=0.5, learning_rate=50.0)
    Y_end = ref.tsne(Y_init, csr, 12.0, 50.0, max_iter=500)[0]
    devs_kl, devs_g = [], []
    for Y in (Y_init, Y_mid, Y_end):
        kl_sk, g_sk = _t_sne._kl_divergence(Y.ravel().copy(), Pc, 1.0, n, 2)
        kl, gr = ref.kl_gradient(Y, csr)
        devs_kl.append(abs(kl - kl_sk) / abs(kl_sk))
        devs_g.append(rel(gr.ravel(), g_sk))
    out.update(Y_mid=Y_mid, Y_end=Y_end, kl_dev=max(devs_kl), grad_dev=max(devs_g))
    # trajectory: restatement vs _gradient_descent after S steps from the init
    traj = []
    for S in (10, 50, 250):
        p_sk, _, _ = _t_sne._gradient_descent(_t_sne._kl_divergence, Y_init.ravel().copy(), 0, S, n_iter_check=10 ** 9,
                                              momentum=0.5, learning_rate=50.0, args=[Pc * 12.0, 1.0, n, 2])
        Yr = ref.descend(Y_init, csr, S, exaggeration=12.0, momentum=0.5, learning_rate=50.0)
        span = float(np.ptp(p_sk))
        traj.append((S, float(np.max(np.abs(Yr.ravel() - p_sk))) / span))
    out.update(traj_steps=np.array([t[0] for t in traj]), traj_dev=np.array([t[1] for t in traj]))
    # finished embedding: scikit-learn's own runs with the reference's parameters
    XF = ref.reference_rows(GOLDEN, N_FINAL)
    ZF = ref.pca(XF, 50)[0]
    kF = min(XF.shape[0] - 1, int(3 * PERPLEXITY + 1))
    assert ref.kth_gap(ZF, kF) >= 1e-9
    iF, dF = ref.neighbors(ZF, kF)
    csrF = ref.symmetrize(iF, ref.binary_search_perplexity(dF, PERPLEXITY)[0])
    kls, tws = [], []
    for angle in (0.5, 0.2):
        for seed in (10, 11, 12):
            E = TSNE(perplexity=PERPLEXITY, early_exaggeration=1.0, random_state=seed, init="pca", learning_rate=2000,
                     angle=angle).fit_transform(ZF).astype(np.float64)
            kls.append(ref.kl_gradient(E, csrF)[0])
            tw = ref.trustworthiness(ZF, E, 12)      # one yardstick for everybody: the restatement's
            assert abs(tw - trustworthiness(ZF, E, n_neighbors=12)) < 1e-3   # (duplicate rows: rank ties fall differently)
            tws.append(tw)
            print("angle %.1f seed %d: KL %.4f trustworthiness %.4f" % (angle, seed, kls[-1], tws[-1]), flush=True)
    out.update(n_final=N_FINAL, final_kl=np.array(kls), final_trust=np.array(tws))
    np.savez_compressed(os.path.join(GOLDEN, "manifold.npz"), **out)
    for key in sorted(out):
        if np.ndim(out[key]) <= 1:
            print(key, out[key])


if __name__ == "__main__":
    main()
