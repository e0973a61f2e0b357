"""tests/kmeans_ref.py, the extended-precision statement tests/test_gpu_kmeans.py holds csrc/kmeans.hip to, on the CPU: it
agrees with the float64 restatements (oracle.kmeans_lloyd_seeded, oracle.kmeans_lloyd) and with scikit-learn on every input
of the GPU file, and those inputs meet the conditions the GPU assertions rest on -- asserted here on the statement alone, so
that no GPU test can pass by leaving a case out."""
import numpy as np
import pytest

from oracle import oracle
from tests import kmeans_ref as ref

MIN_GAP = 1e-6          # device rounding is ~1e-14 relative: above this the labels of a fit are unambiguous
BIG = [s for s in ref.SHAPES if s[0] >= 5]           # the shapes whose fit takes more than two sweeps
STOPPING = [s for s in ref.SHAPES if s[0] >= 5]      # ... and has a stopping tolerance between two of its shifts


def _lloyd_runs(shape):
    """Every phk_kmeans_lloyd whole fit of the GPU file on this shape: (tag, tol_abs, max_iter, the statement's result)."""
    runs = [("zero", 300), ("huge", 300), ("zero", 1), ("zero", 2)] + ([("stop", 300)] if shape in STOPPING else [])
    out = []
    for kind, max_iter in runs:
        tol, result = ref.whole_fit(shape, kind, max_iter)
        out.append(("%s/%d" % (kind, max_iter), tol, max_iter, result))
    return out


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_inputs_are_dyadic_and_exact(shape):
    """Rows are multiples of 1/64 in [-0.5, 8.5], the seed rows are distinct rows of them, and the E-step against the seed
    rows is exact in float64 (exact_gap finds every distance representable)."""
    X, init = ref.shape_input(shape)
    assert X.shape == shape[:2] and init.shape == (shape[2], shape[1])
    assert np.array_equal(X * 64, np.round(X * 64)) and X.min() >= -0.5 and X.max() <= 8.5
    assert len(np.unique(init, axis=0)) == shape[2]
    assert ref.exact_gap(X, init) is not None


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_lloyd_statement_agrees_with_the_float64_restatement(shape):
    """labels, sweeps and empties of kmeans_ref.lloyd_seeded == oracle.kmeans_lloyd_seeded on every whole fit of the GPU
    file, and every such fit keeps its closest call above MIN_GAP."""
    X, init = ref.shape_input(shape)
    for tag, tol, max_iter, (labels, centres, sweeps, empties, gap, shifts) in _lloyd_runs(shape):
        o_labels, o_sweeps, o_empties = oracle.kmeans_lloyd_seeded(X, init, tol, max_iter)
        assert np.array_equal(labels, o_labels), tag
        assert (sweeps, empties) == (o_sweeps, o_empties), tag
        assert len(shifts) == sweeps and centres.shape == init.shape
        assert gap >= MIN_GAP, (tag, gap)
        # the means are those of the final labels wherever the fit converged strictly
        if tag == "zero/300" and sweeps < 300:
            want, sizes = ref.mstep(X, labels, centres)
            assert np.array_equal(want, centres)
    if shape[2] == 1:
        assert ref.whole_fit(shape)[1][4] == ref.INF


@pytest.mark.parametrize("shape", BIG)
def test_capped_fits_need_more_sweeps(shape):
    """max_iter in {1, 2} cuts a fit that needs at least three sweeps; tol = 1e300 stops every fit after one."""
    assert ref.whole_fit(shape)[1][2] >= 3
    for cap in (1, 2):
        assert ref.whole_fit(shape, "zero", cap)[1][2] == cap
    assert ref.whole_fit(shape, "huge")[1][2] == 1


def test_the_extra_e_step_decides_labels_and_gap():
    """What the E-step after the last sweep contributes is visible on these inputs: after one capped sweep it changes labels
    on most shapes, and stepping one sweep at a time meets calls whose second E-step holds the smaller gap."""
    moved, later = [], []
    for shape in BIG:
        X, init = ref.shape_input(shape)
        labels, centres = ref.whole_fit(shape, "zero", 1)[1][:2]
        moved.append(not np.array_equal(labels, ref.estep(X, init)[0]))
        for step in range(ref.whole_fit(shape)[1][2]):
            _, b0, s0 = ref.estep(X, init)
            init = ref.mstep(X, ref.estep(X, init)[0], init)[0]
            _, b1, s1 = ref.estep(X, init)
            later.append(float(ref.gap_of(b1, s1)) + 1e-9 < float(ref.gap_of(b0, s0)))
    assert sum(moved) >= len(BIG) - 1, moved
    assert sum(later) >= 3, later


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_stopping_tolerances_sit_clear_of_every_shift(shape):
    """A fit run with a non-zero tolerance stops at the sweep known in advance -- earlier than the tol = 0 fit --, and no
    shift of it lies within a factor 2 of the tolerance (the device's shift differs from the statement's by rounding only)."""
    found = ref.stopping_tolerance(ref.whole_fit(shape)[1][5])
    assert (found is not None) == (shape in STOPPING)
    if found is None:
        return
    tol, stop_at = found
    got_tol, (labels, centres, sweeps, empties, gap, shifts) = ref.whole_fit(shape, "stop")
    assert got_tol == tol and tol > 0
    assert sweeps == stop_at < ref.whole_fit(shape)[1][2]
    assert all(s > 2 * tol for s in shifts[:-1]) and shifts[-1] * 2 < tol, (tol, shifts)


def test_some_input_meets_empty_clusters():
    """(255, 63, 7) from its random seed rows: clusters run empty, keep their centres and are counted."""
    counts = {shape: ref.whole_fit(shape)[1][3] for shape in ref.SHAPES}
    assert counts[(255, 63, 7)] > 0, counts
    # stepping one sweep at a time meets it too: some step's E-step leaves a cluster without members
    X, init = ref.shape_input((255, 63, 7))
    centres, met = init, 0
    for step in range(ref.whole_fit((255, 63, 7))[1][2]):
        labels, means, _, _ = ref.one_sweep(X, centres, centres)
        empty = np.setdiff1d(np.arange(7), labels)
        assert np.array_equal(means[empty], centres[empty])
        met += len(empty)
        centres = means
    assert met == counts[(255, 63, 7)]
    # and a centre far from every row is empty from the first sweep to the last: it ends as the init row it was
    X, init = ref.far_centre_input()
    labels, centres, sweeps, empties, gap, shifts = ref.lloyd_seeded(X, init, 0.0, 300)
    assert empties == sweeps >= 2 and ref.FAR_CENTRE not in labels and gap >= MIN_GAP
    assert np.array_equal(centres[ref.FAR_CENTRE], init[ref.FAR_CENTRE])
    o_labels, o_sweeps, o_empties = oracle.kmeans_lloyd_seeded(X, init, 0.0)
    assert np.array_equal(labels, o_labels) and (sweeps, empties) == (o_sweeps, o_empties)


@pytest.mark.parametrize("shape", [s for s in ref.SHAPES if s[2] > 1])
def test_first_step_gap_comes_from_the_exact_e_step(shape):
    """One sweep from the dyadic seed rows: the first E-step's gap (exact in float64) is the smaller of the two by more
    than 1e-9, far above the bound of the second -- so the device's min_gap of that call must be that exact value."""
    X, init = ref.shape_input(shape)
    first = ref.exact_gap(X, init)
    labels, means, labels_out, gap = ref.one_sweep(X, init, ref.mstep(X, ref.estep(X, init)[0], init)[0])
    _, best, second = ref.estep(X, means)
    assert first + 1e-9 < float(ref.gap_of(best, second))
    assert abs(float(gap) - first) <= 2.0 ** -53
    assert ref.gap_bound(shape[1]) < 1e-12


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_seeded_fit_statement_agrees_with_the_float64_restatement(shape):
    """kmeans_ref.kmeans_pp_lloyd == oracle.kmeans_lloyd (labels, sweeps; centroids to 1e-12) on the shapes and, at n = 5
    and n = 67, with k = n; closest call above MIN_GAP, no relocation on these rows."""
    X, _ = ref.shape_input(shape)
    for k in [shape[2]] + ([shape[0]] if shape[0] in (5, 67) else []):
        labels, centres, sweeps, relocations, gap = ref.pp_fit(shape, k)
        o_labels, o_centres, o_sweeps = oracle.kmeans_lloyd(X, k, ref.PP_SEED)
        assert np.array_equal(labels, o_labels) and sweeps == o_sweeps, k
        assert np.abs(centres - o_centres).max() <= 1e-12
        assert gap >= MIN_GAP and relocations == 0, (k, gap, relocations)
        if k == shape[0]:
            assert len(np.unique(labels)) == k and np.array_equal(centres[labels], X)


def test_duplicate_rows_relocate_and_meet_the_zero_total_pick():
    """Six points five times each.  k = 6: six clusters of five, no relocation.  k in {7, 10, 30}: after six distinct seeds
    every weight is 0 (the pick is row n - 1), the duplicate centres lose every tie to the lower index, their clusters are
    re-seeded every sweep and only the cap ends the fit -- oracle.kmeans_lloyd does the same."""
    X = ref.duplicate_rows()
    assert X.shape == (30, 3) and len(np.unique(X, axis=0)) == 6
    labels, centres, sweeps, relocations, gap = ref.duplicate_fit(6)
    assert sorted(np.bincount(labels, minlength=6)) == [5] * 6 and relocations == 0 and sweeps < 300
    assert ref.zero_total_picks(X, oracle.kmeans_pp_seeds(X, 6, ref.PP_SEED)) == 0
    for k in ref.DUPLICATE_KS:
        labels, centres, sweeps, relocations, gap = ref.duplicate_fit(k)
        seeds = oracle.kmeans_pp_seeds(X, k, ref.PP_SEED)
        assert ref.zero_total_picks(X, seeds) == k - 6
        assert np.array_equal(seeds[6:], np.repeat(X[-1:], k - 6, axis=0))
        assert relocations >= 1 and sweeps == ref.DUPLICATE_MAX_ITER, (k, relocations, sweeps)
        o_labels, o_centres, o_sweeps = oracle.kmeans_lloyd(X, k, ref.PP_SEED, ref.DUPLICATE_MAX_ITER)
        assert np.array_equal(labels, o_labels) and o_sweeps == sweeps and np.array_equal(centres, o_centres), k


def test_exact_ties():
    """The tie case of the GPU file: the two points at distance 1 from both centres take centre 0, gap exactly 0; and the
    symmetric set on which scikit-learn's own seeds leave exact ties."""
    labels, centres, sweeps, empties, gap, shifts = ref.lloyd_seeded(ref.TIE_X, ref.TIE_INIT, 0.0, 1)
    assert gap == 0.0 and sweeps == 1
    assert ref.estep(ref.TIE_X, ref.TIE_INIT)[0].tolist() == [1, 0, 0, 0]
    assert ref.exact_gap(ref.TIE_X, ref.TIE_INIT) == 0.0
    from phamers_amd import learning
    T = ref.tied_symmetric_set()
    Tc = T - T.mean(axis=0)
    assert np.array_equal(Tc + T.mean(axis=0), T)            # centring is exact
    init, _ = learning.kmeans_plusplus_seeds(Tc, 2, np.random.RandomState(learning.kmeans_seed))
    fit = ref.lloyd_seeded(Tc, init, float(np.mean(np.var(Tc, axis=0)) * 1e-4), 300)
    assert fit[3] == 0 and fit[4] == 0.0


def test_rows_that_are_not_finite_go_to_the_host_fit_without_a_device():
    """A NaN or an infinity among the rows: learning.kmeans_reference_on_device answers None before it touches the device
    (the tolerance it would pass is not a number), and learning.kmeans raises scikit-learn's ValueError."""
    from phamers_amd import learning
    X = ref.shape_input((67, 3, 4))[0].copy()
    for bad in (np.nan, np.inf, -np.inf):
        X[5, 1] = bad
        assert learning.kmeans_reference_on_device(X, 4) is None
        with pytest.raises(ValueError):
            learning.kmeans(X, 4)


@pytest.mark.parametrize("shape", [(257, 65, 7), (1030, 130, 9)])
def test_statement_agrees_with_scikit_learn_from_its_own_seeds(shape):
    """scikit-learn's seeding on the centred rows, its tolerance, then the statement's sweeps: the labels of
    KMeans(n_init=1).fit."""
    from sklearn.cluster import KMeans, kmeans_plusplus
    X, _ = ref.shape_input(shape)
    k = shape[2]
    Xc = X - X.mean(axis=0)
    init, _ = kmeans_plusplus(Xc, k, random_state=np.random.RandomState(10))
    labels, centres, sweeps, empties, gap, shifts = ref.lloyd_seeded(Xc, init, float(np.mean(np.var(Xc, axis=0)) * 1e-4), 300)
    assert empties == 0 and gap >= MIN_GAP
    fit = KMeans(n_clusters=k, random_state=10, n_init=1).fit(X)
    assert np.array_equal(labels, fit.labels_) and sweeps == fit.n_iter_
    o_labels, o_sweeps, o_empties = oracle.kmeans_lloyd_seeded(Xc, init, float(np.mean(np.var(Xc, axis=0)) * 1e-4))
    assert np.array_equal(labels, o_labels) and (sweeps, empties) == (o_sweeps, o_empties)
