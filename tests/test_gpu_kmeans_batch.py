"""The batched k-means core (csrc/kmeans_batch.h) through its three clients, on the GPU: the placement (reference rows plus one
appended row, centred on the fly), the sweep (resident centred rows) and the combo grid (a fold's train rows, centred on the
fly) must agree bit for bit on the same problem; a fit that runs out of sweeps; k = 1; the refusals the core's host half
states once for all three."""
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


# ---- the third client ----------------------------------------------------------------------------------------------------
def _grid_over(X):
    """A ComboGrid whose train set 0 (positive class less fold 0) is exactly X in row order: X is positive and held out by
    fold 1; two more positive rows and three negative ones are held out by fold 0.  -> (grid, set_mean, set_tol)."""
    from phamers_amd import _lib
    rng = np.random.RandomState(len(X))
    D = X.shape[1]
    rows = np.vstack((X, rng.randn(2, D), rng.randn(3, D) + 2.0))
    fold_of = np.r_[np.ones(len(X)), np.zeros(5)].astype(np.uint32)
    positive = np.r_[np.ones(len(X) + 2), np.zeros(3)].astype(np.uint8)
    mean = X.mean(axis=0)
    set_mean, set_tol = np.zeros((4, D)), np.zeros(4)
    set_mean[0], set_tol[0] = mean, np.mean(np.var(X - mean, axis=0)) * 1e-4
    return _lib.ComboGrid(_lib.get_context(), rows, fold_of, positive, 2), set_mean, set_tol


@pytest.mark.parametrize("chunk", ["0", "1", "all but one"])
@pytest.mark.parametrize("shape", SHAPES)
def test_the_combo_grid_agrees_with_the_sweep_bit_for_bit(both, shape, chunk):
    """The same problems -- rows, k, first seed, draws, tolerance -- through phk_combo_grid_fit (rows read through their index
    list, centred on the fly): sweep counts, min_gap and seed_margin as bit patterns and "empty cluster met" equal the sweep's,
    and the bank holds NumPy's mean of X[labels == c] for the sweep's labels, whatever the chunking."""
    from phamers_amd import _lib, learning
    X, ks, _, swept = both[shape]
    chunk = {"0": 0, "1": 1, "all but one": len(ks) - 1}[chunk]
    drawn = [learning.placement_draws(len(X), k) for k in ks]
    bank_off = np.concatenate(([0], np.cumsum(ks)[:-1]))
    grid, set_mean, set_tol = _grid_over(X)
    try:
        out = grid.fit(np.zeros(len(ks)), ks, [d[0] for d in drawn], [d[1] for d in drawn], set_mean, set_tol, int(np.sum(ks)),
                       bank_off, chunk=chunk)
        bank = grid.get_centroids(0, int(np.sum(ks)))
    finally:
        grid.close()
    for i, (k, s) in enumerate(zip(ks, swept)):
        print("n=%d D=%d k=%d chunk=%d: sweeps %d / %d, min_gap %016x / %016x, seed_margin %016x / %016x, empty %s / %s"
              % (shape + (k, chunk, out["n_iter"][i], s["n_iter"], _bits(out["min_gap"][i]).item(), s["min_gap"],
                          _bits(out["seed_margin"][i]).item(), s["seed_margin"], bool(out["status"][i] & _lib.COMBO_GRID_EMPTY),
                          s["empty"])))
        assert int(out["n_iter"][i]) == s["n_iter"], k
        assert _bits(out["min_gap"][i]).item() == s["min_gap"] and _bits(out["seed_margin"][i]).item() == s["seed_margin"], k
        assert bool(out["status"][i] & _lib.COMBO_GRID_EMPTY) == s["empty"], k
        for c in range(k):
            members = X[s["labels"] == c]
            want = np.mean(members, axis=0) if len(members) else np.zeros(X.shape[1])
            assert np.array_equal(_bits(bank[bank_off[i] + c]), _bits(want)), (k, c)


# ---- the refusals the three clients share --------------------------------------------------------------------------------
class _Client(object):
    """One client's handle over `rows` and one problem at a time through it: run(k, first, draws, ...) -> every result array
    as bytes.  `rows_of_problem`: what k and the first seed are measured against (the placement appends a row)."""

    def __init__(self, name, rows):
        from phamers_amd import _lib
        self.name, self.rows = name, rows
        self.rows_of_problem = len(rows) + (1 if name == "placement" else 0)
        self.k_too_large = self.rows_of_problem + 1
        if name == "placement":
            self.handle = _lib.Placement(_lib.get_context(), rows)
        elif name == "sweep":
            self.handle = _lib.Sweep(_lib.get_context(), rows)
        else:
            self.handle, self.set_mean, self.set_tol = _grid_over(rows)

    def run(self, k, first, draws, max_iter=300, chunk=0):
        if self.name == "placement":
            out = self.handle.run(self.rows[:1] + 0.125, k, first, draws, max_iter=max_iter, chunk=chunk)
        elif self.name == "sweep":
            out = self.handle.run([k], [first], [draws], silhouettes=False, max_iter=max_iter, chunk=chunk)
            out = dict(out, seeds=out["seeds"][0], sil=0)
        else:
            out = self.handle.fit([0], [k], [first], [draws], self.set_mean, self.set_tol, max(k, 1), [0], max_iter=max_iter,
                                  chunk=chunk)
            out = dict(out, bank=self.handle.get_centroids(0, max(k, 1)))
        return {key: np.asarray(v).tobytes() for key, v in out.items()}

    def valid(self):
        from phamers_amd import learning
        return self.run(3, *learning.placement_draws(self.rows_of_problem, 3))


CLIENTS = ["placement", "sweep", "combo_grid"]


@pytest.fixture(scope="module")
def clients():
    """(client, "small" | "large") -> (the client over 40 x 3 or 8104 x 1 rows, its valid problem's results), made on demand."""
    made = {}

    def get(name, size):
        if (name, size) not in made:
            rows = _blobs(40, 3, 43) if size == "small" else np.random.RandomState(8104).randn(8104, 1)
            client = _Client(name, rows)
            made[(name, size)] = (client, client.valid())
        return made[(name, size)]
    yield get
    for client, _ in made.values():
        client.handle.close()


@pytest.mark.parametrize("case", ["k = 0", "k too large", "first seed past the rows", "chunk = 65536", "max_iter = 0", "trials"])
@pytest.mark.parametrize("name", CLIENTS)
def test_the_shared_refusals(clients, name, case):
    """kb_check_call / kb_check_problem through each client: ValueError, and the handle then solves a valid problem with the
    bits it gave before.  "trials": k = 8104 needs 2 + int(ln 8104) = 11 seeding trials per centre (e^9 = 8103.08...),
    KB_MAX_TRIALS = 10 are built."""
    from phamers_amd import learning
    client, before = clients(name, "large" if case == "trials" else "small")
    n = client.rows_of_problem
    first, draws = learning.placement_draws(n, 3)
    if case == "k = 0":
        bad = dict(k=0, first=first, draws=np.zeros((0, 2)))
    elif case == "k too large":
        k = client.k_too_large
        bad = dict(k=k, first=first, draws=learning.placement_draws(n, k)[1])
    elif case == "first seed past the rows":
        bad = dict(k=3, first=n, draws=draws)
    elif case == "chunk = 65536":
        bad = dict(k=3, first=first, draws=draws, chunk=65536)
    elif case == "max_iter = 0":
        bad = dict(k=3, first=first, draws=draws, max_iter=0)
    else:
        k = 8104
        assert 2 + int(np.log(k)) == 11 and k <= len(client.rows)
        bad = dict(k=k, first=first, draws=learning.placement_draws(n, k)[1])
    with pytest.raises(ValueError, match="seeding trials" if case == "trials" else None) as err:
        client.run(**bad)
    print("%s, %s: %s" % (name, case, err.value))
    assert client.valid() == before
