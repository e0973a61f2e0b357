"""phamers_amd.manifold on the device against the NumPy restatement (tests/manifold_ref.py), stage by stage, then whole runs.

Tolerances come from tests/golden/manifold.npz (tools/gen_golden_manifold.py): per stage 8 x the deviation the generator
measured between the restatement and scikit-learn in float64 (another summation order over up to n terms), never less than
64 ulp, relative to the stage's largest magnitude; neighbour indices and direct-difference distances are compared for
equality.  The finished embedding must reach scikit-learn's own quality: KL <= the worst of its six runs (angle 0.5 / 0.2,
seeds 10-12) + their spread, trustworthiness >= the worst - their spread."""
import os

import numpy as np
import pytest

from tests import manifold_ref as ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "manifold.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def manifold():
    from phamers_amd import manifold as m
    return m


@pytest.fixture(scope="module")
def stage(gold):
    """The 600 reference rows of the per-stage fixtures and everything the restatement derives from them."""
    X = ref.reference_rows(GOLDEN, int(gold["n_stage"]))
    Z, comps, mean, var = ref.pca(X, 50)
    k = min(X.shape[0] - 1, int(3 * 30.0 + 1))
    idx, d2 = ref.neighbors(Z, k)
    P, beta = ref.binary_search_perplexity(d2, 30.0)
    csr = ref.symmetrize(idx, P)
    Y_init = Z[:, :2] / np.std(Z[:, 0]) * 1e-4
    return dict(X=X, Z=Z, comps=comps, mean=mean, var=var, k=k, idx=idx, d2=d2, P=P, beta=beta, csr=csr, Y_init=Y_init)


def tol(fig):
    return max(8.0 * float(fig), 64.0 * EPS)


def close(got, want, fig, what):
    got, want = np.asarray(got), np.asarray(want)
    scale = float(np.max(np.abs(want)))
    err = float(np.max(np.abs(got - want)))
    print("%s: max deviation %.3e of %.3e (allowed %.3e relative)" % (what, err, scale, tol(fig)))
    assert err <= tol(fig) * scale, (what, err / scale, tol(fig))


def test_pca_against_the_restatement(manifold, stage, gold):
    p = manifold.PCA(50)
    T = p.fit_transform(stage["X"])
    close(p.mean_, stage["mean"], gold["pca_dev_mean"], "mean")
    close(p.explained_variance_, stage["var"], gold["pca_dev_variance"], "explained variance")
    close(p.components_, stage["comps"], gold["pca_dev_components"], "components")
    close(T, stage["Z"], gold["pca_dev_transformed"], "projection")
    assert np.all(p.components_[np.arange(50), np.argmax(np.abs(p.components_), axis=1)] > 0)


def test_neighbours_equal_the_restatement(manifold, stage):
    idx, d2 = manifold.neighbors(stage["Z"], stage["k"])
    assert np.array_equal(idx, stage["idx"])
    assert np.array_equal(d2.view(np.int64), stage["d2"].view(np.int64))


def test_conditional_affinities_and_beta(manifold, stage, gold):
    P, beta = manifold.conditional_affinities(stage["d2"], 30.0)
    close(P, stage["P"], gold["cond_dev"], "conditional P")
    close(beta, stage["beta"], gold["cond_dev"], "beta")
    indptr, cols, vals = manifold.symmetrize(stage["idx"], stage["P"])
    assert np.array_equal(indptr, stage["csr"][0]) and np.array_equal(cols, stage["csr"][1])
    close(vals, stage["csr"][2], gold["joint_dev"], "joint P")
    a = manifold.neighbor_affinities(stage["Z"], 30.0)
    assert np.array_equal(a.indices, stage["idx"])
    close(a.joint()[2], stage["csr"][2], gold["joint_dev"], "joint P through neighbor_affinities")


@pytest.mark.parametrize("which", ["init", "mid", "end"])
def test_objective_and_gradient(manifold, stage, gold, which):
    Y = {"init": stage["Y_init"], "mid": gold["Y_mid"], "end": gold["Y_end"]}[which]
    for ex in (1.0, 12.0):
        kl, g = manifold.kl_gradient(Y, stage["csr"], exaggeration=ex)
        kl_r, g_r = ref.kl_gradient(Y, stage["csr"], ex)
        close([kl], [kl_r], gold["kl_dev"], "KL at %s x%g" % (which, ex))
        close(g, g_r, gold["grad_dev"], "gradient at %s x%g" % (which, ex))


def test_one_update_step(manifold, stage, gold):
    Y = manifold.descend(gold["Y_mid"], stage["csr"], 1, exaggeration=12.0, momentum=0.5, learning_rate=50.0)
    Yr = ref.descend(gold["Y_mid"], stage["csr"], 1, exaggeration=12.0, momentum=0.5, learning_rate=50.0)
    close(Y - gold["Y_mid"], Yr - gold["Y_mid"], gold["grad_dev"], "one update")


def test_trajectory(manifold, stage, gold):
    ok = [i for i in range(len(gold["traj_steps"])) if gold["traj_dev"][i] <= 1e-9]
    assert ok, "no trajectory length with a reference-side deviation <= 1e-9 of the span: %s" % (gold["traj_dev"],)
    S, dev = int(gold["traj_steps"][ok[-1]]), float(gold["traj_dev"][ok[-1]])
    Y = manifold.descend(stage["Y_init"], stage["csr"], S, exaggeration=12.0, momentum=0.5, learning_rate=50.0)
    Yr = ref.descend(stage["Y_init"], stage["csr"], S, exaggeration=12.0, momentum=0.5, learning_rate=50.0)
    err, span = float(np.max(np.abs(Y - Yr))), float(np.ptp(Yr))
    print("S = %d: deviation %.3e of span %.3e (allowed %.3e relative)" % (S, err, span, 8 * dev))
    assert err <= max(8.0 * dev, 64.0 * EPS) * span


@pytest.mark.parametrize("seed,n,d,perplexity", ref.SHAPE_CASES)
def test_shapes(manifold, gold, seed, n, d, perplexity):
    X = ref.synthetic(seed, n, d)
    k = min(n - 1, int(3 * perplexity + 1))
    a = manifold.neighbor_affinities(X, perplexity)
    idx, d2 = ref.neighbors(X, k)
    assert a.indices.shape == (n, k) and np.array_equal(a.indices, idx)
    assert np.array_equal(a.sqdistances.view(np.int64), d2.view(np.int64))
    P, beta = ref.binary_search_perplexity(d2, perplexity)
    close(a.conditional, P, gold["cond_dev"], "conditional P")
    close(a.beta, beta, gold["cond_dev"], "beta")
    csr = ref.symmetrize(idx, P)
    assert np.array_equal(a.joint()[0], csr[0]) and np.array_equal(a.joint()[1], csr[1])
    close(a.joint()[2], csr[2], gold["joint_dev"], "joint P")
    Y = 3.0 * np.random.default_rng(seed).standard_normal((n, 2))
    kl, g = manifold.kl_gradient(Y, csr)
    kl_r, g_r = ref.kl_gradient(Y, csr)
    close([kl], [kl_r], gold["kl_dev"], "KL")
    close(g, g_r, gold["grad_dev"], "gradient")
    Y5, Y5r = manifold.descend(Y, csr, 5), ref.descend(Y, csr, 5)
    # five updates add up at most five gradients' deviations (x 8 covers it; the rounding is not yet amplified)
    close(Y5, Y5r, 8 * float(gold["grad_dev"]), "five steps")
    if d > 2:
        c = min(d, n, 3)
        p = manifold.PCA(c)
        T = p.fit_transform(X)
        Tr, comps, mean, var = ref.pca(X, c)
        close(p.components_, comps, gold["pca_dev_components"], "components")
        close(T, Tr, gold["pca_dev_transformed"], "projection")


def test_several_query_batches_and_column_ranges(manifold, gold):
    """n = 8448, d = 50: the distance rows of the neighbour search take three query batches (256 MiB / (8 n) = 3971 rows,
    cut to 3968) and the gradient 33 column ranges per row block; checked on sampled rows (all of Z enters every row's
    gradient)."""
    seed, n, d, perplexity = ref.LARGE_CASE
    X = ref.synthetic(seed, n, d)
    k = min(n - 1, int(3 * perplexity + 1))
    rows = np.concatenate(([0, 1, 2, 63, 64, 3967, 3968, 3969, n - 3, n - 2, n - 1],
                           np.random.default_rng(0).integers(0, n, 21)))
    a = manifold.neighbor_affinities(X, perplexity)
    idx, d2 = ref.neighbors(X, k, rows)
    assert np.array_equal(a.indices[rows], idx)
    assert np.array_equal(a.sqdistances[rows].view(np.int64), d2.view(np.int64))
    P, beta = ref.binary_search_perplexity(d2, perplexity)
    close(a.conditional[rows], P, gold["cond_dev"], "conditional P")
    csr = a.joint()
    Y = 20.0 * np.random.default_rng(1).standard_normal((n, 2))
    kl, g = manifold.kl_gradient(Y, csr)
    kl_r, g_r = ref.kl_gradient(Y, csr, rows=rows)
    close([kl], [kl_r], gold["kl_dev"], "KL")
    scale = float(np.max(np.abs(g)))
    err = float(np.max(np.abs(g[rows] - g_r)))
    print("gradient on %d sampled rows: %.3e of %.3e" % (len(rows), err, scale))
    assert err <= tol(gold["grad_dev"]) * scale


def test_whole_runs_are_identical_and_reach_scikit_learns_quality(manifold, gold):
    X = ref.reference_rows(GOLDEN, int(gold["n_final"]))
    Z = manifold.PCA(50).fit_transform(X)
    runs = []
    for _ in range(2):
        t = manifold.TSNE(perplexity=30.0, early_exaggeration=1.0, random_state=10, init="pca", learning_rate=2000)
        runs.append((t.fit_transform(Z), t.kl_divergence_, t.n_iter_))
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1:] == runs[1][1:]
    E, kl_dev, n_iter = runs[0]
    Zr = ref.pca(X, 50)[0]
    idx, d2 = ref.neighbors(Zr, 91)
    csr = ref.symmetrize(idx, ref.binary_search_perplexity(d2, 30.0)[0])
    kl = ref.kl_gradient(E, csr)[0]
    tw = ref.trustworthiness(Zr, E, 12)
    kls, tws = gold["final_kl"], gold["final_trust"]
    kl_bound = float(kls.max() + (kls.max() - kls.min()))
    tw_bound = float(tws.min() - (tws.max() - tws.min()))
    print("n_iter %d, KL %.4f (device's own %.4f; bound %.4f), trustworthiness %.4f (bound %.4f)"
          % (n_iter, kl, kl_dev, kl_bound, tw, tw_bound))
    assert abs(kl - kl_dev) <= 1e-3 * abs(kl)     # kl_divergence_ is the objective before the last update, as scikit-learn's
    assert kl <= kl_bound
    assert tw >= tw_bound


def test_scorer_end_to_end(manifold, tmp_path):
    """phamer_scorer.do_tsne on resident counts, save_tsne_data, read_tsne_file."""
    from phamers_amd import _lib, fileIO, phamer
    with np.load(os.path.join(GOLDEN, "ref_features.npz")) as z:
        pos, neg = z["pos_counts"][:150].astype(np.int64), z["neg_counts"][:150].astype(np.int64)
        qry = z["neg_counts"][150:200].astype(np.int64)
    s = phamer.phamer_scorer()
    s.positive_data, s.negative_data = pos / pos.sum(1, keepdims=True), neg / neg.sum(1, keepdims=True)
    s.positive_ids = np.array(["p%d" % i for i in range(150)])
    s.negative_ids = np.array(["n%d" % i for i in range(150)])
    s.data_ids = np.array(["q%d" % i for i in range(50)])
    s._batch = _lib.Batch.from_counts(_lib.get_context(), qry)
    assert s._batch is not None
    s.output_directory = str(tmp_path)
    s.do_tsne()
    assert s.tsne_data.shape == (350, 2) and np.isfinite(s.tsne_data).all()
    assert s.data_points.shape == (50, 256) and s.positive_data.shape == (150, 256)
    all_rows = np.vstack((qry / qry.sum(1, keepdims=True), s.positive_data, s.negative_data))
    Z = manifold.PCA(50).fit_transform(all_rows)
    want = manifold.TSNE(perplexity=30.0, early_exaggeration=1.0, random_state=10, init="pca",
                         learning_rate=2000).fit_transform(Z)
    assert np.array_equal(s.tsne_data, want)
    s.save_tsne_data()
    ids, pts, chops = fileIO.read_tsne_file(s.get_tsne_output_filename())
    assert chops == [50, 150, 150] and ids[:2] == ["q0", "q1"] and ids[50] == "p0" and ids[-1] == "n149"
    assert np.array_equal(pts, s.tsne_data)


def test_input_errors(manifold):
    X = ref.synthetic(1, 40, 3)
    bad = X.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        manifold.TSNE(perplexity=5).fit_transform(bad)
    bad[3, 1] = np.inf
    with pytest.raises(ValueError, match="infinity"):
        manifold.TSNE(perplexity=5).fit_transform(bad)
    with pytest.raises(ValueError, match="perplexity must be less than n_samples"):
        manifold.TSNE(perplexity=40).fit_transform(X)
