"""GPU: the stacked mixture E-step (mixture_sweep.hip) and what is built on it.  The contract is bit
equality: every job of a step call is ``array_equal`` to ``MixtureTable.expect`` on that job's rows alone, for any grouping
under the byte budget, source, order of the jobs and run; every cell of ``mixture.sweep`` equals ``mixture.fit`` field by
field.  Shapes are the smallest that cross the kernels' boundaries (row tile 128, component step 64, row block 1024)."""
import time

import numpy as np
import pytest

from tests import helpers, mixture_ref as mref
from tests.test_gpu_mixture import table_of

pytestmark = pytest.mark.gpu
RB = mref.BLOCK_ROWS
FIELDS = ("log_profiles", "weights", "trace", "n_iter", "converged", "effective_kmers")
# (rows of the set, components): every K and n the issue names, large K on more than one block
MIXED = ((1, 1), (127, 2), (129, 65), (RB - 1, 255), (RB, 17), (RB + 1, 256), (2 * RB + 1, 64))


@pytest.fixture(scope="module")
def golden():
    g = helpers.load_npz("ref_features.npz")
    return g["pos_counts"].astype(np.uint32), g["neg_counts"].astype(np.uint32)


@pytest.fixture(scope="module")
def rows(golden):
    """2 * RB + 1 golden rows, phage and bacterial alternating (the cut of tests/test_gpu_mixture.py)."""
    pos, neg = golden
    n = RB + 1
    out = np.empty((2 * n, 256), dtype=np.uint32)
    out[0::2], out[1::2] = pos[:n], neg[:n]
    return out[:2 * RB + 1]


def single(counts, logp, logw):
    """(T, Nk, L, l) of the single call on ``counts`` alone."""
    from phamers_amd import _lib
    table = _lib.MixtureTable(_lib.get_context(), logp, logw)
    try:
        return table.expect(counts, rows=True)[:4]
    finally:
        table.close()


def step(counts, sets, jobs, resident=False, **kw):
    from phamers_amd import _lib
    ctx = _lib.get_context()
    batch = _lib.Batch.from_counts(ctx, counts) if resident else None
    sweep = _lib.MixtureSweep(ctx, batch if resident else counts, sets)
    try:
        return sweep.step(jobs, **kw)
    finally:
        sweep.close()
        if batch is not None:
            batch.close()


def same(a, b):
    return len(a) == len(b) and all((x is None and y is None) or np.array_equal(x, y) for p, q in zip(a, b) for x, y in zip(p, q))


@pytest.fixture(scope="module")
def mixed(rows):
    """dict(sets, jobs, want, got): seven jobs over seven non-contiguous row sets (the last one all rows), the single call's
    answer per job and the default step call's."""
    rng = np.random.RandomState(5)
    sets = [np.sort(rng.choice(len(rows), n, replace=False)) for n, _ in MIXED]
    assert np.array_equal(sets[-1], np.arange(len(rows))) and all((np.diff(s) > 1).any() for s in sets[1:-1])
    jobs = [(i,) + table_of(rows, K, seed=i) for i, (_, K) in enumerate(MIXED)]
    want = [single(rows[sets[s]], lp, lw) for s, lp, lw in jobs]
    return dict(sets=sets, jobs=jobs, want=want, got=step(rows, sets, jobs, rows=True))


# ---- 1. one mixed call ---------------------------------------------------------------------------------------------------------
def test_every_job_of_a_mixed_call_is_the_single_call(mixed):
    for (n, K), got, want in zip(MIXED, mixed["got"], mixed["want"]):
        assert got[0].shape == (K, 256) and got[1].shape == (K,) and got[3].shape == (n,)
        for g, w in zip(got, want):
            assert np.array_equal(g, w), (n, K)


def test_every_job_of_a_mixed_call_is_inside_the_bound(rows, mixed):
    for (s, lp, lw), (T, Nk, L, l) in zip(mixed["jobs"], mixed["got"]):
        ratio = mref.check_e_step(dict(T=T, Nk=Nk, L=L, l=l), rows[mixed["sets"][s]], lp, lw)
        print("n=%d K=%d worst error / bound: %.4f" % (len(l), len(Nk), ratio))


# ---- 2. invariances ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("budget", [1, 6 << 20, 64 << 20])
def test_no_result_depends_on_the_grouping(rows, mixed, budget):
    """1 byte: every job a group of its own; 6 MiB: the jobs in several groups; 64 MiB: one group."""
    assert same(step(rows, mixed["sets"], mixed["jobs"], rows=True, _budget_bytes=budget), mixed["got"])


def test_resident_batch_repeated_runs_and_job_order(rows, mixed):
    from phamers_amd import _lib
    ctx = _lib.get_context()
    batch = _lib.Batch.from_counts(ctx, rows)
    sweep = _lib.MixtureSweep(ctx, batch, mixed["sets"])
    try:
        assert same(sweep.step(mixed["jobs"], rows=True), mixed["got"])
        assert same(sweep.step(mixed["jobs"], rows=True), mixed["got"])
        order = [3, 6, 0, 5, 1, 4, 2]
        got = sweep.step([mixed["jobs"][i] for i in order], rows=True, _budget_bytes=6 << 20)
        assert same(got, [mixed["got"][i] for i in order])
        assert same(sweep.step(mixed["jobs"][5:6], rows=True), mixed["got"][5:6])
    finally:
        sweep.close()
        batch.close()


# ---- 3. widths -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,resident", [(4, True), (64, True), (30, False), (1024, True), (320, False), (258, False)])
def test_other_widths(D, resident):
    """D > 256: more than one column group per row block (the descriptor's y).  1024: four groups; 320: two, and three
    waves of the second leave at once; 258: the scalar loaders, two live columns in the second group."""
    rng = np.random.RandomState(D)
    counts = np.stack([rng.multinomial(2500, rng.dirichlet(np.full(D, 0.7))) for _ in range(131)]).astype(np.uint32)
    sets = [np.arange(131), np.sort(rng.choice(131, 77, replace=False))]
    jobs = [(0,) + table_of(counts, 5, seed=D), (1,) + table_of(counts, 70, seed=D)]
    got = step(counts, sets, jobs, resident=resident, rows=True)
    for (s, lp, lw), g in zip(jobs, got):
        assert same([g], [single(counts[sets[s]], lp, lw)])
        mref.check_e_step(dict(T=g[0], Nk=g[1], L=g[2], l=g[3]), counts[sets[s]], lp, lw)


# ---- 3b. a job of two fold levels beside jobs of one ---------------------------------------------------------------------------
TWO_LEVELS = 256 * RB + 1


@pytest.fixture(scope="module")
def levels():
    """dict(counts, sets, jobs, want, got): 256 RB + 3 rows at D = 4; set 0 all rows (aliases the source), set 1 all but two
    interior rows (257 blocks, gathered), set 2 129 scattered rows.  Fold descriptors of the default call (one group), from
    phk_mix_sweep_step: level 0 holds 2 + 2 + 2 + 1 (two blocks of vectors for each big job, two element blocks for
    K = 65), level 1 one per big job, which writes into the result area while the small jobs have left the list."""
    started = time.perf_counter()
    counts, logp, logw = mref.two_profile_case(TWO_LEVELS + 2, 2)
    rng = np.random.RandomState(11)
    sets = [np.arange(len(counts)), np.delete(np.arange(len(counts)), [1000, 200 * RB + 7]),
            np.sort(rng.choice(len(counts), 129, replace=False))]
    assert len(sets[1]) == TWO_LEVELS and (np.diff(sets[2]) > 1).any()
    small = counts[sets[2]]
    jobs = [(1, logp, logw), (2,) + table_of(small, 65, seed=1), (0,) + mref.two_profile_case(TWO_LEVELS + 2, 1)[1:],
            (2,) + table_of(small, 2, seed=2)]
    want = [single(counts[sets[s]], lp, lw) for s, lp, lw in jobs]
    got = step(counts, sets, jobs, rows=True)
    print("levels fixture: %.2f s" % (time.perf_counter() - started))
    return dict(counts=counts, sets=sets, jobs=jobs, want=want, got=got)


def test_a_two_level_job_beside_one_level_jobs_is_the_single_call(levels):
    started = time.perf_counter()
    assert same(levels["got"], levels["want"])
    counts, sets = levels["counts"], levels["sets"]
    # the gathered job: N_k and L in the device's order over its own r and l, everything inside the bound
    _, lp, lw = levels["jobs"][0]
    T, Nk, L, l = levels["got"][0]
    from phamers_amd import _lib
    table = _lib.MixtureTable(_lib.get_context(), lp, lw)
    try:
        r, l_single = table.responsibilities(counts[sets[1]])
    finally:
        table.close()
    Nk_want, L_want = mref.device_order(r, l_single)
    assert np.array_equal(l, l_single) and np.array_equal(Nk, Nk_want) and L == L_want and (Nk >= TWO_LEVELS / 8.0).all()
    print("worst error / bound: %.4f" % mref.check_e_step(dict(T=T, Nk=Nk, L=L, l=l), counts[sets[1]], lp, lw))
    # the aliasing job, K = 1: exact
    T, Nk, L, l = levels["got"][2]
    assert np.array_equal(T[0], counts.sum(axis=0, dtype=np.uint64).astype(np.float64)) and Nk[0] == float(len(counts))
    assert L == mref.device_order(np.ones((len(counts), 1)), l)[1]
    print("two-level sweep job: %.2f s" % (time.perf_counter() - started))


@pytest.mark.parametrize("variant", ["own_groups", "mixed_levels_per_group", "reversed", "resident"])
def test_two_level_jobs_do_not_depend_on_grouping_order_or_source(levels, variant):
    """own_groups: a budget of 1 byte, every job alone; mixed_levels_per_group: 200 MiB lies between one big job's buffers
    (128 MiB of R) and two, so each group holds a two-level job and a one-level job."""
    started = time.perf_counter()
    counts, sets, jobs, want = (levels[k] for k in ("counts", "sets", "jobs", "want"))
    if variant == "own_groups":
        got = step(counts, sets, jobs, rows=True, _budget_bytes=1)
    elif variant == "mixed_levels_per_group":
        got = step(counts, sets, jobs, rows=True, _budget_bytes=200 << 20)
    elif variant == "reversed":
        got = step(counts, sets, jobs[::-1], rows=True)[::-1]
    else:
        got = step(counts, sets, jobs, resident=True, rows=True)
    assert same(got, want)
    print("%s: %.2f s" % (variant, time.perf_counter() - started))


# ---- 4. edge cases -------------------------------------------------------------------------------------------------------------
def test_dead_components_beside_a_live_job_and_a_row_without_counts(rows):
    counts = rows[:200].copy()
    counts[7] = 0
    sets = [np.arange(3, 200, 2)]
    dead = table_of(rows, 20, seed=1, dead=(0, 13, 19))
    live = table_of(rows, 20, seed=2)
    got = step(counts, sets, [(0,) + dead, (0,) + live], rows=True)
    assert same(got, [single(counts[sets[0]], *dead), single(counts[sets[0]], *live)])
    T, Nk, L, l = got[0]
    assert not T[[0, 13, 19]].any() and not Nk[[0, 13, 19]].any() and np.isfinite(T).all() and np.isfinite(l).all()
    assert np.isfinite(L) and abs(l[2]) < 1e-13   # row 7, the set's third, has no counts: l = log of the weights' sum


def test_evaluation_mode_returns_the_rows_alone(rows, mixed):
    got = step(rows, mixed["sets"], mixed["jobs"], rows=True, expect=False, _budget_bytes=6 << 20)
    for g, w in zip(got, mixed["got"]):
        assert g[0] is None and g[1] is None and g[2] is None and np.array_equal(g[3], w[3])
    plain = step(rows, mixed["sets"], mixed["jobs"])
    assert all(p[3] is None for p in plain) and same([p[:3] for p in plain], [w[:3] for w in mixed["got"]])


def test_empty_job_list_and_refusals(rows):
    from phamers_amd import _lib
    ctx = _lib.get_context()
    sweep = _lib.MixtureSweep(ctx, rows[:50], [np.arange(50), np.arange(0, 50, 3)])
    try:
        assert sweep.step([]) == []
        good, bad = table_of(rows, 4), table_of(rows, 6)
        bad[0][2, 9] = np.nan
        with pytest.raises(ValueError, match="job 1"):
            sweep.step([(0,) + good, (1,) + bad])
        with pytest.raises(ValueError, match="job 2"):
            sweep.step([(0,) + good, (1,) + good, (0, good[0], np.array([0.0, np.inf, 0.0, 0.0]))])
        with pytest.raises(ValueError):
            sweep.step([(2,) + good])
        with pytest.raises(ValueError):
            sweep.step([(0, good[0], np.full(4, -np.inf))])   # every weight 0
        assert same(sweep.step([(1,) + good], rows=True), [single(rows[:50][::3], *good)])   # still usable
    finally:
        sweep.close()
    for sets in ([np.array([3, 2])], [np.array([0, 50])], [np.zeros(0, dtype=np.int64)]):
        with pytest.raises(ValueError):
            _lib.MixtureSweep(ctx, rows[:50], sets)


# ---- 5. mixture.sweep ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    return mref.planted(7, 3, 100, 400, 1.0)[0]


def assert_same_mixture(a, b):
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


def test_sweep_cells_equal_fit_and_choose_three(planted):
    from phamers_amd import cross_validate, mixture
    Ks, folds, n_init = [2, 3, 4], 4, 2
    sw = mixture.sweep(planted, Ks, folds=folds, fold_seed=0, seed=0, n_init=n_init, max_iter=60)
    fold_of = cross_validate.FoldPlan(len(planted), 0, folds, 0).positive
    for K in Ks:
        for f in list(range(folds)) + [None]:
            train = planted if f is None else planted[fold_of != f]
            for i in range(n_init):
                assert_same_mixture(sw.mixture(K, init=i, fold=f), mixture.fit(train, K, seed=i, max_iter=60))
            best = mixture.fit(train, K, seed=0, n_init=n_init, max_iter=60)
            assert_same_mixture(sw.mixture(K, fold=f), best)
            if f is not None:
                held = np.flatnonzero(fold_of == f)
                assert np.array_equal(sw.held_out_log_likelihood[Ks.index(K), held], best.log_likelihood(planted[held]))
    assert np.isfinite(sw.held_out_log_likelihood).all()
    assert sw.best('bic') == 3 and sw.best('held_out') == 3


# ---- 6. two classes ------------------------------------------------------------------------------------------------------------
def test_cross_validate_equals_the_loop_of_fit_and_score(golden):
    from phamers_amd import compare, cross_validate, learning, likelihood, mixture
    pos, neg = golden[0][:300], golden[1][:300]
    Ks, folds = [4, 16], 3
    res = mixture.cross_validate(pos, neg, Ks, folds, seed=0, fit_seed=0, max_iter=30)
    plan = cross_validate.FoldPlan(300, 300, folds, 0)
    for a, K in enumerate(Ks):
        want = np.full(600, np.nan)
        for f in range(folds):
            mp = mixture.fit(pos[plan.positive != f], K, seed=0, max_iter=30)
            mn = mixture.fit(neg[plan.negative != f], K, seed=0, max_iter=30)
            hp, hn = np.flatnonzero(plan.positive == f), np.flatnonzero(plan.negative == f)
            want[hp] = mixture.score(pos[hp], mp, mn)
            want[300 + hn] = mixture.score(neg[hn], mp, mn)
        assert np.array_equal(res.scores[a], want)
        assert res.auc[a] == learning.predictor_performance(want[:300], want[300:])[2]
        assert res.accuracy[a] == likelihood.evaluate(want[:300], want[300:])[1]
    assert compare.mixture_cells(res)[0].shape == (2, 600)


# ---- 7. command line -----------------------------------------------------------------------------------------------------------
def test_mixture_grid_two_class_mode(golden, tmp_path):
    from phamers_amd import fileIO, mixture, mixture_grid
    pos, neg = golden[0][:120], golden[1][:120]
    for name, c in (("pos.csv", pos), ("neg.csv", neg)):
        fileIO.save_counts(c, ["r%d" % i for i in range(len(c))], str(tmp_path / name))
    out = tmp_path / "grid.csv"
    assert mixture_grid.main(["-pf", str(tmp_path / "pos.csv"), "-nf", str(tmp_path / "neg.csv"), "-K", "2", "5", "-N", "3",
                              "--seed", "0", "--max_iter", "20", "-out", str(out)]) == 0
    columns, table = mixture_grid.read_grid(str(out))
    assert columns == mixture_grid.TWO_CLASS_COLUMNS and [row["K"] for row in table] == [2, 5]
    res = mixture.cross_validate(pos, neg, [2, 5], 3, seed=0, max_iter=20, bic=True)
    for b, row in enumerate(table):
        for name in columns[1:]:
            assert row[name] == getattr(res, name)[b], name
        assert 0.5 < row["auc"] <= 1.0 and np.isfinite(row["bic_positive"]) and row["held_out_per_kmer_positive"] < 0
