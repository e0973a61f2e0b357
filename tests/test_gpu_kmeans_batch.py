"""The batched k-means core (csrc/kmeans_batch.h) through its two clients, on the GPU: the placement (reference rows plus one
appended row, centred on the fly) and the sweep (resident centred rows) must agree bit for bit on the same problem; a fit that
runs out of sweeps; k = 1."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(65, 17), (257, 33), (130, 256)]


def _blobs(n, D, seed):
    """tests/test_gpu_placement.py's odd-shape rows: six seeded blobs."""
    rng = np.random.RandomState(seed)
    centres = rng.uniform(-1, 1, (6, D))
    return centres[rng.randint(0, 6, n)] + 0.3 * rng.randn(n, D)


def _ks(n):
    """2 + int(ln k) seeding trials per centre: 2, 2, 3, 3, 5 and, where the rows allow it, 6."""
    return [1, 2, 5, 7, 32] + ([55] if n > 65 else [])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _lloyd(X, rows, max_iter=300):
    """phk_kmeans_lloyd on NumPy's centred rows from the given seed rows -> (labels, sweeps, empty clusters, min_gap)."""
    from phamers_amd import _lib
    Xc = np.ascontiguousarray(X - X.mean(axis=0))
    init = np.ascontiguousarray(Xc[np.asarray(rows, dtype=np.int64)])
    tol_abs = float(np.mean(np.var(Xc, axis=0)) * 1e-4)
    labels = np.empty(Xc.shape[0], dtype=np.uint32)
    n_iter, n_empty, gap = ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
    ctx = _lib.get_context()
    _lib.check(ctx.lib.phk_kmeans_lloyd(ctx.handle, _lib.ptr(Xc), Xc.shape[0], Xc.shape[1], len(rows), _lib.ptr(init), tol_abs,
                                        int(max_iter), None, _lib.ptr(labels), ctypes.byref(n_iter), ctypes.byref(n_empty),
                                        ctypes.byref(gap)))
    return labels, n_iter.value, n_empty.value, gap.value


def _placed(X, k, seed=None, **kw):
    """One problem through the placement: the last row is the appended one."""
    from phamers_amd import _lib, learning
    first, draws = learning.placement_draws(len(X), k) if seed is None else learning.placement_draws(len(X), k, seed)
    pl = _lib.Placement(_lib.get_context(), X[:-1])
    try:
        out = pl.run(X[-1:], k, first, draws, **kw)
    finally:
        pl.close()
    return {"labels": out["labels"][0], "seeds": out["seeds"][0], "n_iter": int(out["n_iter"][0]),
            "min_gap": _bits(out["min_gap"][0]).item(), "seed_margin": _bits(out["seed_margin"][0]).item(),
            "empty": bool(out["status"][0] & _lib.PLACEMENT_EMPTY)}


def _swept(X, ks, seeds=None, **kw):
    """The problems (ks[i], seeds[i]) through the sweep, in one call."""
    from phamers_amd import _lib, learning
    drawn = [learning.placement_draws(len(X), k) if seeds is None else learning.placement_draws(len(X), k, seeds[i])
             for i, k in enumerate(ks)]
    sw = _lib.Sweep(_lib.get_context(), X)
    try:
        out = sw.run(ks, [d[0] for d in drawn], [d[1] for d in drawn], silhouettes=False, **kw)
    finally:
        sw.close()
    return [{"labels": out["labels"][i], "seeds": out["seeds"][i], "n_iter": int(out["n_iter"][i]),
             "min_gap": _bits(out["min_gap"][i]).item(), "seed_margin": _bits(out["seed_margin"][i]).item(),
             "empty": bool(out["status"][i] & _lib.SWEEP_EMPTY)} for i in range(len(ks))]


def _same(a, b):
    return (np.array_equal(a["seeds"], b["seeds"]) and np.array_equal(a["labels"], b["labels"]) and a["n_iter"] == b["n_iter"]
            and a["min_gap"] == b["min_gap"] and a["seed_margin"] == b["seed_margin"] and a["empty"] == b["empty"])


@pytest.fixture(scope="module")
def both():
    """(n, D) -> (rows, ks, the placement's results one call per k, the sweep's results from one call)."""
    out = {}
    for n, D in SHAPES:
        X = _blobs(n, D, n + D)
        ks = _ks(n)
        out[(n, D)] = (X, ks, [_placed(X, k) for k in ks], _swept(X, ks))
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_the_two_clients_agree_bit_for_bit(both, shape):
    """Seeds, labels, sweep counts, "empty cluster met", and min_gap and seed_margin as bit patterns: both sides perform the
    same operations on the same values, ties and empty clusters included.  (D = 1 is left out: NumPy sums one column
    pairwise, which only the sweep reproduces.  The two stopping tolerances come from different host formulas, equal to
    ~1e-10 relative: a final shift between the two values would show as another sweep count.)"""
    X, ks, placed, swept = both[shape]
    for k, p, s in zip(ks, placed, swept):
        print("n=%d D=%d k=%d: sweeps %d / %d, seeds equal %s, min_gap %016x / %016x, seed_margin %016x / %016x, empty %s / %s"
              % (shape + (k, p["n_iter"], s["n_iter"], np.array_equal(p["seeds"], s["seeds"]), p["min_gap"], s["min_gap"],
                          p["seed_margin"], s["seed_margin"], p["empty"], s["empty"])))
        assert np.array_equal(p["seeds"], s["seeds"]), k
        assert np.array_equal(p["labels"], s["labels"]), k
        assert p["n_iter"] == s["n_iter"], k
        assert p["min_gap"] == s["min_gap"] and p["seed_margin"] == s["seed_margin"], k
        assert p["empty"] == s["empty"], k


@pytest.mark.parametrize("shape", SHAPES)
def test_one_centre(both, shape):
    """k = 1 through both clients against phk_kmeans_lloyd: one label, the same sweep count, no gap and no seeding decision."""
    X, ks, placed, swept = both[shape]
    inf = _bits(np.inf).item()
    for got in (placed[ks.index(1)], swept[ks.index(1)]):
        labels, n_iter, n_empty, gap = _lloyd(X, got["seeds"])
        assert gap == np.inf and n_empty == 0 and not labels.any()
        assert not got["labels"].any() and got["n_iter"] == n_iter
        assert got["min_gap"] == inf and got["seed_margin"] == inf and not got["empty"]


@pytest.fixture(scope="module")
def unfinished():
    """140 x 33, k = 5: the first seed of the draws whose fit takes the single-problem path at least 3 sweeps, and the first
    k = 2 fit on the same rows that is over within 2 (13 of the seeds 10 ... 1033 give one, 47 the first)."""
    X = _blobs(140, 33, 140 + 33)
    seeds = list(range(10, 74))
    five = _swept(X, [5] * len(seeds), seeds)
    long_seed = next((s for s, r in zip(seeds, five) if _lloyd(X, r["seeds"])[1] >= 3), None)
    assert long_seed is not None
    two = _swept(X, [2] * len(seeds), seeds)
    short_seed, short = next(((s, r) for s, r in zip(seeds, two) if r["n_iter"] <= 2), (None, None))
    assert short_seed is not None
    print("k = 5 seed %s; k = 2 seed %s" % (long_seed, short_seed))
    return X, long_seed, short_seed, short


@pytest.mark.parametrize("max_iter", [1, 2])
def test_running_out_of_sweeps(unfinished, max_iter):
    """A problem that neither converged nor met the tolerance when the sweeps ran out: max_iter sweeps, then the final E-step,
    as phk_kmeans_lloyd does with the same max_iter from the device's own seeds.  Beside it in the sweep's chunk a k = 2
    problem that is over within 2 sweeps keeps its results: a finished and an unfinished problem in one chunk."""
    X, long_seed, short_seed, short = unfinished
    mixed = max_iter == 2
    swept = _swept(X, [5, 2] if mixed else [5], [long_seed, short_seed] if mixed else [long_seed], max_iter=max_iter)
    for got in (_placed(X, 5, long_seed, max_iter=max_iter), swept[0]):
        labels, n_iter, _, gap = _lloyd(X, got["seeds"], max_iter)
        print("max_iter %d: sweeps %d / %d, min_gap %016x / %016x" % (max_iter, got["n_iter"], n_iter, got["min_gap"], _bits(gap).item()))
        assert n_iter == max_iter and got["n_iter"] == max_iter
        assert np.array_equal(got["labels"], labels)
        assert got["min_gap"] == _bits(gap).item()
    if mixed:
        assert _same(swept[1], short)
