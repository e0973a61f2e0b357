"""The k-means sweep on the GPU (phk_sweep_run, learning.kmeans_sweep, cluster.silhouette_curve): parity with the reference's
fits (tests/golden/sweep.npz), which problems the device keeps, equality with the single-problem device paths, invariance
under batching, odd shapes, the declined problems, seeds, the path past the pair-distance budget, the curve."""
import ctypes

import numpy as np
import pytest

from oracle import oracle
from tests import helpers, sweep_ref

pytestmark = pytest.mark.gpu

SETS = ("phage", "s24", "s130")


@pytest.fixture(scope="module")
def golden():
    g = helpers.load_npz("sweep.npz")
    ref = helpers.load_npz("ref_features.npz")
    data = {"phage": oracle.normalize_counts(ref["pos_counts"].astype(np.int64))}
    for name in SETS[1:]:
        data[name] = g[name + "_Xq"].astype(np.float64) / float(g[name + "_scale"][0])
    return g, data


@pytest.fixture(scope="module")
def swept(golden):
    """One kmeans_sweep call per set over the fixture's (k, seed) grid: name -> (records, details)."""
    from phamers_amd import learning
    g, data = golden
    out = {}
    for name in SETS:
        ks = list(dict.fromkeys(g[name + "_k"].tolist()))
        seeds = list(dict.fromkeys(g[name + "_seed"].tolist()))
        details = {}
        recs = learning.kmeans_sweep(data[name], ks, seeds=seeds, _details=details)
        assert [(r["k"], r["seed"]) for r in recs] == list(zip(g[name + "_k"].tolist(), g[name + "_seed"].tolist()))
        out[name] = (recs, details)
    return out


def _single(X, k, seed, rows=None):
    """The single-problem device path with its results unpacked: learning.kmeans_reference_on_device's steps (host seeding
    -- or the given seed rows --, phk_kmeans_lloyd) -> (labels, sweeps, empty clusters, min_gap, seed rows)."""
    from phamers_amd import _lib, learning
    Xc = np.array(X, dtype=np.float64, order="C")
    Xc -= Xc.mean(axis=0)
    if rows is None:
        init, rows = learning.kmeans_plusplus_seeds(Xc, int(k), np.random.RandomState(seed))
    else:
        init = Xc[np.asarray(rows, dtype=np.int64)]
    init = np.ascontiguousarray(init, dtype=np.float64)
    tol_abs = float(np.mean(np.var(Xc, axis=0)) * 1e-4)
    labels = np.empty(Xc.shape[0], dtype=np.uint32)
    n_iter, n_empty, gap = ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
    ctx = _lib.get_context()
    _lib.check(ctx.lib.phk_kmeans_lloyd(ctx.handle, _lib.ptr(Xc), Xc.shape[0], Xc.shape[1], int(k), _lib.ptr(init), tol_abs, 300, None,
                                        _lib.ptr(labels), ctypes.byref(n_iter), ctypes.byref(n_empty), ctypes.byref(gap)))
    return labels.astype(np.int32), n_iter.value, n_empty.value, gap.value, np.asarray(rows)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name", SETS)
def test_parity_with_the_reference_fits(golden, swept, name):
    """1. labels and sweep counts equal scikit-learn's, the mean silhouette within 1e-8 (Gram form against
    direct differences), whatever route a problem took."""
    g, _ = golden
    recs, details = swept[name]
    for i, r in enumerate(recs):
        err = abs(r["silhouette"] - g[name + "_sil"][i])
        print("%s k=%d seed=%d route %s sweeps %d seed margin %.3g (restated %.3g) gap %.3g (restated %.3g) silhouette err %.3g"
              % (name, r["k"], r["seed"], r["route"], r["n_iter"], details["seed_margin"][i], g[name + "_margin"][i],
                 details["min_gap"][i], g[name + "_gap"][i], err))
        assert np.array_equal(r["labels"], g[name + "_labels"][i].astype(np.int32)), (name, r["k"], r["seed"], r["route"])
        assert r["n_iter"] == g[name + "_n_iter"][i]
        assert r["silhouettes"].shape == r["labels"].shape and r["silhouette"] == float(np.mean(r["silhouettes"]))
        assert err <= 1e-8
    if name == "phage":   # k = 300 and 590 have singleton clusters: silhouette 0 there
        assert g["phage_singletons"][-1] > 0
        sizes = np.bincount(recs[-1]["labels"])
        assert np.all(recs[-1]["silhouettes"][sizes[recs[-1]["labels"]] == 1] == 0.0)


@pytest.mark.parametrize("name", SETS)
def test_the_device_keeps_every_problem_clear_of_its_guards(golden, swept, name):
    """2. The device's and the restatement's roundings differ by under 2e-12 relative, so a problem whose
    restated seeding margin is >= 1e-8 and restated gap >= 1e-7 -- 100 x the guards -- cannot trip them: device route.
    The generator refuses synthetic cases below those figures, so every synthetic problem qualifies."""
    g, _ = golden
    recs, _ = swept[name]
    clear = (g[name + "_margin"] >= 1e-8) & (g[name + "_gap"] >= 1e-7)
    if name != "phage":
        assert clear.all()
    print(name, "clear of the guards:", int(clear.sum()), "of", len(recs), "routes:", [r["route"] for r in recs])
    for i, r in enumerate(recs):
        if clear[i]:
            assert r["route"] == "device", (name, r["k"], r["seed"])


@pytest.mark.parametrize("name", SETS)
def test_equal_to_the_single_problem_paths(golden, swept, name):
    """3. For every problem on the device route: labels, sweeps and seeds equal the single-problem path's, min_gap and the
    per-row silhouettes bit for bit (the sweep keeps phk_silhouettes' summation order)."""
    from phamers_amd import learning
    _, data = golden
    recs, details = swept[name]
    X = data[name]
    checked = 0
    for i, r in enumerate(recs):
        if r["route"] != "device":
            continue
        labels, n_iter, n_empty, gap, rows = _single(X, r["k"], r["seed"])
        assert n_empty == 0
        assert np.array_equal(r["labels"], labels) and r["n_iter"] == n_iter
        got = learning.kmeans_reference_on_device(X, r["k"], seed=r["seed"])
        assert got is not None and np.array_equal(got[0], r["labels"]) and got[1] == r["n_iter"]
        assert _bits(details["min_gap"][i]) == _bits(gap), (details["min_gap"][i], gap)
        assert np.array_equal(details["seeds"][i], rows)
        assert np.array_equal(_bits(r["silhouettes"]), _bits(learning.silhouettes(X, r["labels"])))
        checked += 1
    assert checked >= len(recs) - 2


def test_batch_invariance_bit_for_bit(golden):
    """4. The same problems alone, in one call, reversed, with a k listed twice and in chunks of 3: identical results.  The
    set mixes k = 2 with k = n - 1: seeding ends at different steps and the problems stop in different sweeps."""
    from phamers_amd import _lib
    _, data = golden
    X = data["s24"]
    n = X.shape[0]
    ks = [2, n - 1, 5, 13, 50, 8, 3]
    drawn = {k: sweep_ref.draws(n, k, 10) for k in ks}
    sw = _lib.Sweep(_lib.get_context(), X)

    def run(order, **kw):
        out = sw.run(order, [drawn[k][0] for k in order], [drawn[k][1] for k in order], **kw)
        return [{"labels": out["labels"][i].copy(), "n_iter": int(out["n_iter"][i]), "gap": _bits(out["min_gap"][i]).item(),
                 "margin": _bits(out["seed_margin"][i]).item(), "sil": _bits(out["sil"][i]).copy(), "seeds": out["seeds"][i].copy(),
                 "status": int(out["status"][i])} for i in range(len(order))]

    def same(a, b):
        return (np.array_equal(a["labels"], b["labels"]) and a["n_iter"] == b["n_iter"] and a["gap"] == b["gap"]
                and a["margin"] == b["margin"] and np.array_equal(a["sil"], b["sil"]) and np.array_equal(a["seeds"], b["seeds"])
                and a["status"] == b["status"])
    try:
        together = run(ks)
        alone = [run([k])[0] for k in ks]
        backwards = run(ks[::-1])[::-1]
        twice = run(ks + [13])
        chunked = run(ks, chunk=3)
    finally:
        sw.close()
    sweeps = [r["n_iter"] for r in together]
    print("sweeps:", sweeps)
    assert len(set(sweeps)) > 1
    for i, k in enumerate(ks):
        assert same(together[i], alone[i]), k
        assert same(together[i], backwards[i]), k
        assert same(together[i], twice[i]), k
        assert same(together[i], chunked[i]), k
    assert same(twice[-1], together[ks.index(13)])


@pytest.mark.parametrize("n", [3, 63, 64, 65, 257])
def test_shapes(n):
    """5. n around the tile and workgroup sizes, D around the LDS step and at 256, k = 2, n - 1 and one in between, random
    rows: against the restatement and the single-problem paths.  With so few rows per centre many of these fits hold an
    EXACT seeding tie (two trial rows that are each other's nearest uncovered neighbour give the same potential whichever is
    chosen): the restatement reports margin 0 there, the device must report a margin below the guard, and the seeds are
    compared only where the restatement is clear of it.  Lloyd and the silhouettes are compared in every case, from the
    seeds the device chose."""
    from phamers_amd import _lib, learning
    seeds_compared = 0
    for D in (1, 15, 16, 17, 256):
        X = np.random.RandomState(1000 * n + D).randn(n, D)
        Xc = sweep_ref.centre(X)
        ks = sorted({2, n - 1, max(2, n // 3)})
        drawn = [sweep_ref.draws(n, k, 10) for k in ks]
        sw = _lib.Sweep(_lib.get_context(), X)
        try:
            out = sw.run(ks, [d[0] for d in drawn], [d[1] for d in drawn])
        finally:
            sw.close()
        for i, k in enumerate(ks):
            rows, margin = sweep_ref.kmeans_plusplus(Xc, k, 10)
            print("n=%d D=%d k=%d restated margin %.3g; device margin %.3g gap %.3g status %d sweeps %d"
                  % (n, D, k, margin, out["seed_margin"][i], out["min_gap"][i], out["status"][i], out["n_iter"][i]))
            if margin >= 1e-8:
                assert out["seed_margin"][i] >= learning.SEED_MIN_MARGIN
                assert np.array_equal(out["seeds"][i], rows)
                assert abs(out["seed_margin"][i] - margin) <= 1e-9 * max(1.0, margin)
                seeds_compared += 1
            elif margin == 0.0:
                assert out["seed_margin"][i] < learning.SEED_MIN_MARGIN
            dev_rows = out["seeds"][i].astype(np.int64)
            assert len(set(dev_rows.tolist())) == k or out["seed_margin"][i] == 0.0
            labels, n_iter, n_empty, gap, _ = _single(X, k, 10, rows=dev_rows)
            assert np.array_equal(out["labels"][i], labels) and out["n_iter"][i] == n_iter
            assert _bits(out["min_gap"][i]) == _bits(gap) and bool(out["status"][i]) == bool(n_empty)
            ref_labels, ref_iter, ref_gap, ref_empty = sweep_ref.lloyd(Xc, dev_rows)
            if ref_gap >= 1e-7 and not ref_empty:
                assert np.array_equal(out["labels"][i], ref_labels) and out["n_iter"][i] == ref_iter
                assert abs(out["min_gap"][i] - ref_gap) <= 1e-9 * max(1.0, ref_gap)
            if len(set(labels.tolist())) == k:
                assert np.array_equal(_bits(out["sil"][i]), _bits(learning.silhouettes(X, labels)))
                # against NumPy's direct differences: both sides sum the same n non-negative distances, each within
                # (D + 2) u of exact, in some order: (n + 2 D + 4) u relative per cluster mean, through (b - a) / max(a, b)
                # under 6 x that
                assert np.max(np.abs(out["sil"][i] - sweep_ref.silhouettes(X, labels))) <= 8 * (n + 2 * D + 4) * 2.0 ** -53
    assert seeds_compared >= 3


def test_declined_problems_take_the_host_route():
    """6. Two pairs of bit-identical rows and k = n - 1: once the n - 2 distinct rows are centres the potential is 0 with a
    centre still to draw -- an exact seeding tie (margin 0), and a cluster that runs empty.  Route 'host', scikit-learn's
    results.  A NaN row is a ValueError."""
    import warnings
    from sklearn.cluster import KMeans
    from sklearn.metrics import silhouette_samples
    from phamers_amd import learning
    X = np.random.RandomState(3).randn(40, 6)
    X[7], X[9] = X[3], X[5]
    ref = sweep_ref.kmeans(X, 39, 10)
    assert ref["seed_margin"] == 0.0 or ref["n_empty"] > 0
    details = {}
    recs = learning.kmeans_sweep(X, [4, 39], _details=details)
    print("routes", [r["route"] for r in recs], "margins", details["seed_margin"], "gaps", details["min_gap"], "status", details["status"])
    assert recs[1]["route"] == "host" and (details["seed_margin"][1] < learning.SEED_MIN_MARGIN or details["status"][1])
    for r in recs:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            fit = KMeans(n_clusters=r["k"], random_state=10).fit(X)
        assert np.array_equal(r["labels"], fit.labels_) and r["n_iter"] == fit.n_iter_
        assert np.max(np.abs(r["silhouettes"] - silhouette_samples(X, fit.labels_))) <= 1e-8
    bad = X.copy()
    bad[11, 2] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        learning.kmeans_sweep(bad, [4])


def test_the_host_fit_on_request(monkeypatch, golden):
    from phamers_amd import learning
    g, data = golden
    monkeypatch.setenv("PHAMERS_KMEANS", "sklearn")
    i = g["s130_k"].tolist().index(7)
    recs = learning.kmeans_sweep(data["s130"], [7], seeds=[int(g["s130_seed"][i])])
    assert recs[0]["route"] == "host" and np.array_equal(recs[0]["labels"], g["s130_labels"][i]) and recs[0]["n_iter"] == g["s130_n_iter"][i]
    assert abs(recs[0]["silhouette"] - g["s130_sil"][i]) <= 1e-8


def test_seeds(golden):
    """7. seeds=[10, 11]: two different label sets, each scikit-learn's for its seed."""
    from sklearn.cluster import KMeans
    from phamers_amd import learning
    _, data = golden
    X = data["s24"]
    recs = learning.kmeans_sweep(X, [8], seeds=[10, 11])
    assert [(r["k"], r["seed"]) for r in recs] == [(8, 10), (8, 11)]
    assert not np.array_equal(recs[0]["labels"], recs[1]["labels"])
    for r in recs:
        assert np.array_equal(r["labels"], KMeans(n_clusters=8, random_state=r["seed"]).fit(X).labels_)
        assert r["route"] == "device"


def test_past_the_pair_budget(golden):
    """8. With a budget of 0 bytes for the stored pair distances every problem takes phk_silhouettes' own pass: same bits."""
    from phamers_amd import learning
    _, data = golden
    X = data["s24"]
    ks = [2, 13, 50, 299]
    stored = learning.kmeans_sweep(X, ks)
    passes = learning.kmeans_sweep(X, ks, _pair_budget=0)
    for a, b in zip(stored, passes):
        assert a["route"] == b["route"] == "device"
        assert np.array_equal(a["labels"], b["labels"]) and np.array_equal(_bits(a["silhouettes"]), _bits(b["silhouettes"]))


def test_silhouette_curve(golden):
    """9. The reference's grid clipped to n - 1 on the 300-row set.  Every repeat is the same fit, and with two repeats the
    reference's arithmetic is exact (x + x and its half): std == 0 and the means are the fits' mean silhouettes -- item
    1's, where the grid meets the fixture.  With the reference's five repeats 3 x and 5 x round: there the curve must be
    what np.mean / np.std give for five copies."""
    from phamers_amd import cluster, learning
    g, data = golden
    X = data["s24"]
    grid = np.arange(10, 600, 10)
    grid = grid[grid <= X.shape[0] - 1]
    recs = learning.kmeans_sweep(X, grid)
    ks, mean, std = cluster.silhouette_curve(X, grid, num_repeats=2)
    assert np.array_equal(ks, grid) and len(ks) == 29
    assert np.all(std == 0.0)
    assert np.array_equal(_bits(mean), _bits([r["silhouette"] for r in recs]))
    met = 0
    for i in range(len(g["s24_k"])):
        if g["s24_seed"][i] == 10 and g["s24_k"][i] in grid:
            assert abs(mean[grid.tolist().index(g["s24_k"][i])] - g["s24_sil"][i]) <= 1e-8
            met += 1
    assert met >= 1
    ks5, mean5, std5 = cluster.silhouette_curve(X, grid)
    for i, r in enumerate(recs):
        five = np.zeros(5)
        five[:] = r["silhouette"]
        assert mean5[i] == np.mean(five) and std5[i] == np.std(five)
