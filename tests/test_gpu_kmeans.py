"""csrc/kmeans.hip on the GPU -- phk_kmeans_lloyd (the default route of learning.kmeans, and the fit the batched core is held
to bit for bit) and phk_kmeans -- against tests/kmeans_ref.py, the same algorithms in extended precision: labels, sweep
counts, empty clusters, the returned centres and min_gap, at the smallest shapes that cross each boundary of the kernels, on
exact ties, at both stopping rules, on duplicate rows (empty-cluster re-seeding, the zero-total pick) and at the entries'
argument checks.  tests/test_kmeans_host.py asserts, on the statement alone, the conditions these comparisons rest on.

The two tolerances (derived in kmeans_ref.centre_bound and kmeans_ref.gap_bound, neither from device output):
  centres : |got - want| <= (m_c + 2) 2^-53 max_i |X[i, d]| per coordinate, m_c the cluster's size -- a sequential float64 sum
            of m_c terms and one division;
  min_gap : |got - want| <= 2 (D + 10) 2^-53 absolute for E-steps at the same float64 centres -- best and second are sums of
            at most D non-negative terms under at most D + 8 roundings each, their ratio is <= 1, one subtraction and one
            division follow.
"""
import ctypes

import numpy as np
import pytest

from tests import kmeans_ref as ref

pytestmark = pytest.mark.gpu

MANY = [s for s in ref.SHAPES if s[2] > 1]      # the shapes with a second centre
BIG = [s for s in ref.SHAPES if s[0] >= 5]      # ... whose fit takes at least three sweeps and has a stopping tolerance


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _lloyd_rc(X, n, D, k, init, tol, max_iter, centres, labels):
    """phk_kmeans_lloyd's return code, arguments as given."""
    from phamers_amd import _lib
    ctx = _lib.get_context()
    n_iter, n_empty, gap = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_double(-1.0)
    rc = ctx.lib.phk_kmeans_lloyd(ctx.handle, _lib.ptr(X), n, D, k, _lib.ptr(init), tol, max_iter, _lib.ptr(centres),
                                  _lib.ptr(labels), ctypes.byref(n_iter), ctypes.byref(n_empty), ctypes.byref(gap))
    return rc, n_iter.value, n_empty.value, gap.value


def _lloyd(X, init, tol, max_iter=300):
    """-> (labels, centres_out, n_iter, n_empty, min_gap) of phk_kmeans_lloyd."""
    from phamers_amd import _lib
    X, init = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(init, dtype=np.float64)
    labels = np.full(X.shape[0], 0xFFFFFFFF, dtype=np.uint32)
    centres = np.full(init.shape, np.nan)
    rc, n_iter, n_empty, gap = _lloyd_rc(X, X.shape[0], X.shape[1], init.shape[0], init, float(tol), int(max_iter), centres, labels)
    _lib.check(rc)
    return labels.astype(np.int64), centres, n_iter, n_empty, gap


def _assert_centres(got, want, X, labels, tag):
    """Within kmeans_ref.centre_bound of the statement's; a cluster without members in `labels` got its centre in an earlier
    sweep from at most n rows."""
    sizes = np.bincount(labels, minlength=len(want))
    bound = ref.centre_bound(X, labels, len(want))
    bound[sizes == 0] = (len(X) + 2.0) * 2.0 ** -53 * np.abs(X).max(axis=0)
    err = np.abs(got - want)
    print("%s: centres' largest error / bound = %.3f" % (tag, (err / bound).max()))
    assert (err <= bound).all(), (tag, float((err / bound).max()))


@pytest.fixture(scope="module")
def fits():
    """(shape, tol kind, max_iter) -> (the statement's tolerance and result, the device's result), each fit run once."""
    done = {}

    def get(shape, kind="zero", max_iter=300):
        key = (shape, kind, max_iter)
        if key not in done:
            X, init = ref.shape_input(shape)
            tol, want = ref.whole_fit(shape, kind, max_iter)
            done[key] = (tol, want, _lloyd(X, init, tol, max_iter))
        return done[key]
    return get


@pytest.mark.parametrize("kind", ["zero", "stop"])
@pytest.mark.parametrize("shape", ref.SHAPES)
def test_lloyd_whole_fits(fits, shape, kind):
    """From seed rows with tol = 0, and with a tolerance between two consecutive shifts of that fit (it then stops at a sweep
    known in advance, followed by the extra E-step): labels, n_iter and n_empty equal the statement, centres_out lies within
    the summation bound."""
    if kind == "stop" and shape not in BIG:
        assert ref.whole_fit(shape, "stop") is None      # (a one-sweep fit has no two shifts to stop between)
        return
    X, init = ref.shape_input(shape)
    tol, (labels, centres, sweeps, empties, gap, shifts), (g_labels, g_centres, g_iter, g_empty, g_gap) = fits(shape, kind)
    tag = "%s %s tol=%g" % (shape, kind, tol)
    print("%s: sweeps %d / %d, empties %d / %d, min_gap %.17g / %.17g" % (tag, g_iter, sweeps, g_empty, empties, g_gap, gap))
    assert (g_iter, g_empty) == (sweeps, empties), tag
    assert np.array_equal(g_labels, labels), tag
    _assert_centres(g_centres, centres, X, labels, tag)
    if shape[2] == 1:
        assert g_gap == np.inf and not g_labels.any()
    # (min_gap of a whole fit is printed only: the device's centres drift from the statement's by rounding from the second
    # sweep on, so it is held to its bound one sweep at a time, below)


def test_lloyd_empty_cluster_keeps_its_centre():
    """A centre far from every row has no member in any sweep: counted once per sweep, and returned as the init row it was,
    bit for bit, while the other centres are their clusters' means."""
    X, init = ref.far_centre_input()
    labels, centres, sweeps, empties, gap, shifts = ref.lloyd_seeded(X, init, 0.0, 300)
    g_labels, g_centres, g_iter, g_empty, g_gap = _lloyd(X, init, 0.0)
    assert (g_iter, g_empty) == (sweeps, empties) and g_empty == g_iter
    assert np.array_equal(g_labels, labels)
    assert np.array_equal(_bits(g_centres[ref.FAR_CENTRE]), _bits(init[ref.FAR_CENTRE]))
    _assert_centres(g_centres, centres, X, labels, "far centre")


@pytest.mark.parametrize("shape", MANY)
def test_lloyd_min_gap_one_sweep_at_a_time(fits, shape):
    """max_iter = 1, tol = 0, centres_out fed back as init: every call is two E-steps (against init, against the returned
    centres) and one M-step, and the statement is evaluated at the device's own centres, so each step stands alone.
    min_gap within 2 (D + 10) 2^-53 of the statement's at every step; bit-equal on the first step, whose deciding E-step is
    exact in float64 (dyadic rows against dyadic centres); an empty cluster's centre is its init row bit for bit; stepping
    to convergence gives the whole fit's labels."""
    X, init = ref.shape_input(shape)
    n, D, k = shape
    whole = fits(shape)[2]
    bound = ref.gap_bound(D)
    centres, labels_out = init, None
    for step in range(ref.whole_fit(shape)[1][2]):
        g_labels, g_centres, g_iter, g_empty, g_gap = _lloyd(X, centres, 0.0, 1)
        labels_in, means, labels_out, gap = ref.one_sweep(X, centres, g_centres)
        print("%s step %d: min_gap %.17g, statement %.17g, difference / bound = %.3f"
              % (shape, step, g_gap, float(gap), abs(ref.LD(g_gap) - gap) / bound))
        assert g_iter == 1
        assert abs(ref.LD(g_gap) - gap) <= bound, (step, g_gap, float(gap))
        if step == 0:
            assert _bits(g_gap) == _bits(ref.exact_gap(X, init)), (g_gap, ref.exact_gap(X, init))
        assert np.array_equal(g_labels, labels_out), step
        _assert_centres(g_centres, means, X, labels_in, "%s step %d" % (shape, step))
        empty = np.setdiff1d(np.arange(k), labels_in)
        assert g_empty == len(empty)
        assert np.array_equal(_bits(g_centres[empty]), _bits(centres[empty])), step
        centres = g_centres
        if np.array_equal(labels_in, labels_out):
            break
    assert np.array_equal(labels_out, whole[0])


def test_lloyd_exact_ties_and_one_centre():
    """Two points at distance exactly 1 from both centres: ties keep the lower centre index and the gap is exactly 0.  One
    centre: every label 0, gap inf."""
    want = ref.lloyd_seeded(ref.TIE_X, ref.TIE_INIT, 0.0, 1)
    g_labels, g_centres, g_iter, g_empty, g_gap = _lloyd(ref.TIE_X, ref.TIE_INIT, 0.0, 1)
    tied = ref.estep(ref.TIE_X, ref.TIE_INIT)[0]
    assert tied.tolist() == [1, 0, 0, 0]
    _assert_centres(g_centres, want[1], ref.TIE_X, tied, "ties")       # centre 0 is the mean of the three, the tied two included
    assert np.array_equal(g_centres[1], ref.TIE_X[0]) and np.allclose(g_centres[0], [4.0 / 3, 1.0 / 3], rtol=0, atol=1e-15)
    assert np.array_equal(g_labels, want[0]) and (g_iter, g_empty) == (1, 0)
    assert g_gap == 0.0 and want[4] == 0.0
    X, _ = ref.shape_input((67, 3, 4))
    want = ref.lloyd_seeded(X, X[:1], 0.0, 300)
    g_labels, g_centres, g_iter, g_empty, g_gap = _lloyd(X, X[:1], 0.0)
    assert not g_labels.any() and g_gap == np.inf and (g_iter, g_empty) == (want[2], 0) and want[4] == np.inf
    _assert_centres(g_centres, want[1], X, want[0], "k = 1")


def test_tied_fit_goes_to_the_host():
    """learning.kmeans_reference_on_device on a symmetric set whose seeds leave points exactly between the two centres
    answers None (min_gap = 0 < KMEANS_MIN_GAP), and learning.kmeans then returns scikit-learn's labels."""
    from sklearn.cluster import KMeans
    from phamers_amd import learning
    T = ref.tied_symmetric_set()
    assert learning.kmeans_reference_on_device(T, 2) is None
    Tc = T - T.mean(axis=0)
    init, _ = learning.kmeans_plusplus_seeds(Tc, 2, np.random.RandomState(learning.kmeans_seed))
    assert _lloyd(Tc, init, float(np.mean(np.var(Tc, axis=0)) * 1e-4))[3:] == (0, 0.0)
    assert np.array_equal(learning.kmeans(T, 2), KMeans(n_clusters=2, random_state=learning.kmeans_seed).fit(T).labels_)


@pytest.mark.parametrize("shape", BIG)
def test_lloyd_stopping_rules(fits, shape):
    """tol = 1e300: one sweep, then the extra E-step -- the labels are those against the returned centres, not the sweep's.
    max_iter in {1, 2} on a fit that needs more: n_iter = max_iter and, again after the extra E-step, the statement's labels."""
    X, init = ref.shape_input(shape)
    for kind, cap in (("huge", 300), ("zero", 1), ("zero", 2)):
        tol, (labels, centres, sweeps, empties, gap, shifts), (g_labels, g_centres, g_iter, g_empty, g_gap) = fits(shape, kind, cap)
        tag = "%s tol=%g max_iter=%d" % (shape, tol, cap)
        assert g_iter == sweeps == (1 if kind == "huge" else cap), tag
        assert g_empty == empties, tag
        assert np.array_equal(g_labels, labels), tag
        assert np.array_equal(g_labels, ref.estep(X, g_centres)[0]), tag
        # the returned centres are the means of the last sweep's own labels: those against the centres one sweep earlier
        before = init if sweeps == 1 else ref.whole_fit(shape, "zero", 1)[1][1]
        _assert_centres(g_centres, centres, X, ref.estep(X, before)[0], tag)


def _seeded_cases():
    return [(s, s[2]) for s in ref.SHAPES] + [(s, s[0]) for s in ref.SHAPES if s[0] in (5, 67)]


@pytest.mark.parametrize("shape,k", _seeded_cases())
def test_seeded_fit(shape, k):
    """phk_kmeans through learning.kmeans_gpu: k-means++ seeds by the slice-sum walk (n below, just past and far past its
    256 slices), Lloyd sweeps; k = n puts every row in its own cluster.  Labels and sweeps equal the statement, centroids
    within the summation bound, and a second call returns the same bits."""
    from phamers_amd import learning
    X, _ = ref.shape_input(shape)
    labels, centres, sweeps, relocations, gap = ref.pp_fit(shape, k)
    g_labels, g_centres, g_sweeps = learning.kmeans_gpu(X, k, seed=ref.PP_SEED)
    assert g_sweeps == sweeps and np.array_equal(g_labels, labels), (shape, k)
    _assert_centres(g_centres, centres, X, labels, "%s k=%d" % (shape, k))
    if k == shape[0]:
        assert np.array_equal(g_centres[g_labels], X)
    again = learning.kmeans_gpu(X, k, seed=ref.PP_SEED)
    assert np.array_equal(again[0], g_labels) and np.array_equal(_bits(again[1]), _bits(g_centres)) and again[2] == g_sweeps


@pytest.mark.parametrize("k", (6,) + ref.DUPLICATE_KS)
def test_seeded_fit_on_duplicate_rows(k):
    """Six points five times each.  k = 6 converges with six clusters of five.  k > 6: the seeding runs out of weight (all
    remaining distances 0: the pick is row n - 1), the duplicate centres lose every tie, and their empty clusters take the
    farthest point of a cluster of size > 1, ties to the lower index, every sweep until max_iter -- labels, sweeps and
    centroids (every sum is exact here) equal the statement, relocations included."""
    from phamers_amd import learning
    X = ref.duplicate_rows()
    labels, centres, sweeps, relocations, gap = ref.duplicate_fit(k)
    cap = 300 if k == 6 else ref.DUPLICATE_MAX_ITER
    g_labels, g_centres, g_sweeps = learning.kmeans_gpu(X, k, seed=ref.PP_SEED, max_iter=cap)
    print("k=%d: sweeps %d / %d, relocations in the statement %d" % (k, g_sweeps, sweeps, relocations))
    assert g_sweeps == sweeps and np.array_equal(g_labels, labels), k
    assert np.array_equal(_bits(g_centres), _bits(centres)), k
    if k == 6:
        assert np.bincount(g_labels, minlength=6).tolist() == [5] * 6 and g_sweeps < cap
        assert np.array_equal(g_centres[g_labels], X)
    else:
        assert g_sweeps == cap and relocations >= 1


def test_refusals():
    """PHK_ERR_ARG from both entries for k = 0, k > n, D = 0, max_iter = 0, a NULL X and a NULL output they cannot do without
    (phk_kmeans: centroids -- its labels may be NULL; phk_kmeans_lloyd: init, labels), and from phk_kmeans_lloyd for a
    negative or NaN tol.  Nothing is written, and the context still fits afterwards."""
    from phamers_amd import _lib
    ctx = _lib.get_context()
    X, init = ref.shape_input((67, 3, 4))
    X, init = np.ascontiguousarray(X), np.ascontiguousarray(init)
    n, D, k = 67, 3, 4
    labels = np.full(n, 7, dtype=np.uint32)
    centres = np.full((k, D), -1.0)
    good = dict(X=X, n=n, D=D, k=k, init=init, tol=0.0, max_iter=300, centres=centres, labels=labels)
    bad = [dict(k=0), dict(k=n + 1), dict(n=0), dict(D=0), dict(max_iter=0), dict(max_iter=-1), dict(tol=-1e-300),
           dict(tol=float("nan")), dict(tol=-np.inf), dict(X=None), dict(init=None), dict(labels=None)]
    for change in bad:
        a = dict(good, **change)
        rc = _lloyd_rc(a["X"], a["n"], a["D"], a["k"], a["init"], a["tol"], a["max_iter"], a["centres"], a["labels"])
        assert rc == (_lib.PHK_ERR_ARG, -1, -1, -1.0), (change, rc)
        assert "phk_kmeans_lloyd" in ctx.lib.phk_last_error().decode()
    n_iter = ctypes.c_int(-1)
    for change in [dict(k=0), dict(k=n + 1), dict(n=0), dict(D=0), dict(max_iter=0), dict(max_iter=-1), dict(X=None),
                   dict(centres=None)]:
        a = dict(good, **change)
        rc = ctx.lib.phk_kmeans(ctx.handle, _lib.ptr(a["X"]), a["n"], a["D"], a["k"], ref.PP_SEED, a["max_iter"],
                                _lib.ptr(a["centres"]), _lib.ptr(a["labels"]), ctypes.byref(n_iter))
        assert rc == _lib.PHK_ERR_ARG and n_iter.value == -1, (change, rc)
        assert "phk_kmeans:" in ctx.lib.phk_last_error().decode()
    assert (labels == 7).all() and (centres == -1.0).all()
    want = ref.whole_fit((67, 3, 4))[1]
    got = _lloyd(X, init, 0.0)
    assert np.array_equal(got[0], want[0]) and got[2] == want[2]


def test_a_nan_row_is_refused_by_the_facade():
    """A row with NaN (or an infinity) through learning.kmeans raises scikit-learn's ValueError, as the reference's fit does:
    the device route hands the fit to the host -- its tolerance, the mean column variance, is not a number, which
    phk_kmeans_lloyd refuses -- and the host fit refuses the row.  Given a valid tolerance the entry itself runs such rows to
    the end: the centred column is NaN, no distance compares, every point stays with centre 0, the other clusters are
    reported empty in every sweep and there is no gap."""
    from phamers_amd import learning
    X = ref.shape_input((67, 3, 4))[0].copy()
    X[5, 1] = np.nan
    for bad in (np.nan, np.inf):
        X[5, 1] = bad
        assert learning.kmeans_reference_on_device(X, 4) is None
        with pytest.raises(ValueError):
            learning.kmeans(X, 4)
    X[5, 1] = np.nan
    Xc = X - X.mean(axis=0)
    g_labels, g_centres, g_iter, g_empty, g_gap = _lloyd(Xc, Xc[:4], 0.0)
    assert not g_labels.any() and g_empty == 3 * g_iter and g_gap == np.inf
