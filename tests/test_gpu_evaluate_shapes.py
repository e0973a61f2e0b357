"""The radix argsort, the integer ROC curve and the truth table (phamers_amd/csrc/evaluate.hip) past the shapes
tests/test_gpu_evaluate.py reaches: every small n, the drop rule's first cases, the edges of the curve's workgroup partition,
raw label bytes, the resident (_dev) entries, passes skipped between passes that run, workgroups of two and three tiles, and a
truth table past one grid stride.  All of it is integer-exact: every assertion is equality with the NumPy statement
tests/evaluate_ref.py (roc_points, truth_counts) or with the stable NumPy argsort."""
import ctypes

import numpy as np
import pytest

from tests import evaluate_ref

pytestmark = pytest.mark.gpu

TILE, MAX_BLOCKS = 4096, 512          # PHK_SORT_TILE, PHK_SORT_MAX_BLOCKS
ROC_THREADS, ROC_BLOCKS = 256, 1024   # EV_THREADS, EV_ROC_BLOCKS


def _assert_curve(got, want):
    assert got[0].dtype == np.uint64 and np.array_equal(got[0], want[0]), "fps"
    assert got[1].dtype == np.uint64 and np.array_equal(got[1], want[1]), "tps"
    assert np.array_equal(got[2], want[2]), "thresholds"
    assert type(got[3]) is int and got[3] == want[3], "area2"


def _curve_both_ways(scores, labels):
    from phamers_amd import learning
    for drop in (True, False):
        want = evaluate_ref.roc_points(scores, labels, drop)
        try:
            _assert_curve(learning.roc_points(scores, labels, drop), want)
        except AssertionError as e:
            raise AssertionError("n=%d drop=%s: %s" % (len(scores), drop, e))
    return want


def _raw_roc(scores, label_bytes, drop):
    """phk_roc_curve on the label bytes as they are (learning.roc_points makes them 0 / 1 first)."""
    from phamers_amd import _lib
    ctx = _lib.get_context()
    x = np.ascontiguousarray(scores, dtype=np.float64)
    lab = np.ascontiguousarray(label_bytes, dtype=np.uint8)
    n = len(x)
    fps, tps, thr = np.empty(n + 1, np.uint64), np.empty(n + 1, np.uint64), np.empty(n + 1, np.float64)
    m, area2 = ctypes.c_uint64(), ctypes.c_uint64()
    _lib.check(ctx.lib.phk_roc_curve(ctx.handle, _lib.ptr(x), _lib.ptr(lab), n, 1 if drop else 0, _lib.ptr(fps), _lib.ptr(tps),
                                     _lib.ptr(thr), ctypes.byref(m), ctypes.byref(area2)))
    return fps[:m.value].copy(), tps[:m.value].copy(), thr[:m.value].copy(), int(area2.value)


def _raw_truth(scores, label_bytes, threshold):
    """phk_truth_counts on the scores and label bytes as they are (learning.truth_counts takes two finite classes)."""
    from phamers_amd import _lib
    ctx = _lib.get_context()
    x = np.ascontiguousarray(scores, dtype=np.float64)
    lab = np.ascontiguousarray(label_bytes, dtype=np.uint8)
    counts = np.full(4, 99, dtype=np.uint64)
    _lib.check(ctx.lib.phk_truth_counts(ctx.handle, _lib.ptr(x), _lib.ptr(lab), len(x), float(threshold), _lib.ptr(counts)))
    return tuple(int(c) for c in counts)


def _truth_statement(scores, label_bytes, threshold):
    pos = np.asarray(label_bytes) != 0
    return evaluate_ref.truth_counts(scores[pos], scores[~pos], threshold)


# ---- 1. every small n ------------------------------------------------------------------------------------------------------------
SMALL_N = list(range(1, 71)) + [255, 256, 257, 511, 512, 513]


def _pattern(kind, rng, n):
    if kind == "distinct":
        return rng.permutation(n) * 0.25 - 3.0
    if kind == "two_valued":
        return rng.choice([-1.0, 1.0], n)
    values = rng.permutation(n)[:n] * 0.5 - 2.0                      # "runs": few values, each held by 1 .. 5 elements
    x = np.repeat(values, rng.randint(1, 6, n))[:n]
    return x[rng.permutation(n)]


@pytest.mark.parametrize("kind", ["distinct", "two_valued", "runs"])
def test_every_small_n(kind):
    """n = 1 .. 70 and around one and two workgroups of the curve's passes; labels at random places (the positives do not
    come first), both settings of drop_intermediate."""
    rng = np.random.RandomState(len(kind))
    sizes_of_curves, empty_class = set(), 0
    for n in SMALL_N:
        x = _pattern(kind, rng, n)
        assert x.shape == (n,)
        labels = (rng.rand(n) < 0.5).astype(np.uint8)
        k = int(labels.sum())
        if n >= 16:
            assert 0 < k < n and int(labels[:k].sum()) < k           # both classes, and the positives do not come first
        empty_class += k in (0, n)
        want = _curve_both_ways(x, labels)
        sizes_of_curves.add(len(want[0]) - 1)
    assert empty_class >= 1                                          # (n = 1 at the least)
    if kind != "two_valued":
        assert {1, 2, 3, 4, 5}.issubset(sizes_of_curves)             # run counts around the drop rule's m1 <= 2


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 64, 256, 257])
@pytest.mark.parametrize("label", [0, 1])
def test_small_n_with_an_empty_class(n, label):
    rng = np.random.RandomState(n)
    labels = np.full(n, label, dtype=np.uint8)
    for x in (rng.permutation(n) + 0.5, np.round(rng.normal(0, 1, n), 1), np.zeros(n)):
        want = _curve_both_ways(x, labels)
        assert want[3] == 0 and int(want[1 - label][-1]) == 0 and int(want[label][-1]) == n


# ---- 2. the drop rule's first cases ------------------------------------------------------------------------------------------------
def _runs(*runs):
    """scores and labels from (positives, negatives) per run of equal scores, highest score first, negatives first within a
    run (so no positives-first order helps)."""
    scores, labels = [], []
    for r, (p, q) in enumerate(runs):
        scores += [float(len(runs) - r)] * (p + q)
        labels += [0] * q + [1] * p
    return np.array(scores), np.array(labels, dtype=np.uint8)


DROP_CASES = {
    # name: (runs, the points (fps, tps) the curve keeps under drop_intermediate, after (0, 0))
    "m1=3 middle collinear": ([(1, 1), (1, 1), (1, 1)], [(1, 1), (3, 3)]),
    "m1=3 middle not collinear": ([(1, 1), (2, 0), (1, 1)], [(1, 1), (1, 3), (2, 4)]),
    "m1=3 collinear in one count only": ([(1, 1), (1, 2), (1, 1)], [(1, 1), (3, 2), (4, 3)]),
    "m1=4 both inner collinear": ([(1, 1), (1, 1), (1, 1), (1, 1)], [(1, 1), (4, 4)]),
    "m1=4 first inner collinear": ([(1, 1), (1, 1), (1, 1), (2, 1)], [(1, 1), (3, 3), (4, 5)]),
    "m1=4 second inner collinear": ([(1, 1), (2, 1), (1, 1), (1, 1)], [(1, 1), (2, 3), (4, 5)]),
    "m1=3 all positive": ([(1, 0), (1, 0), (1, 0)], [(0, 1), (0, 3)]),
    "m1=3 all negative": ([(0, 2), (0, 2), (0, 2)], [(2, 0), (6, 0)]),
    "m1=3 all positive, uneven": ([(1, 0), (2, 0), (1, 0)], [(0, 1), (0, 3), (0, 4)]),
    "m1=2": ([(1, 1), (1, 1)], [(1, 1), (2, 2)]),
}


@pytest.mark.parametrize("name", sorted(DROP_CASES))
def test_drop_rule_first_cases(name):
    from phamers_amd import learning
    runs, kept = DROP_CASES[name]
    scores, labels = _runs(*runs)
    order = np.random.RandomState(len(name)).permutation(len(scores))          # and the rows in no particular order
    scores, labels = scores[order], labels[order]
    want = _curve_both_ways(scores, labels)                                    # (returns the statement without dropping)
    assert len(want[0]) - 1 == len(runs)
    fps, tps, thr, area2 = learning.roc_points(scores, labels, True)
    assert list(zip(fps.tolist(), tps.tolist())) == [(0, 0)] + kept            # by hand, not only by the statement
    assert area2 == want[3] and thr[0] == np.inf and thr[-1] == 1.0


# ---- 3. the edges of the curve's workgroup partition ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [ROC_BLOCKS * ROC_THREADS - 1, ROC_BLOCKS * ROC_THREADS, ROC_BLOCKS * ROC_THREADS + 1])
def test_partition_edges_at_scale(n):
    """1024 workgroups with ranges of 255 / 256, 256 and 256 / 257 elements; a run of ties longer than three whole ranges in
    the middle of the order and one that ends on the last element; labels interleaved."""
    rng = np.random.RandomState(n % 1000)
    x = rng.normal(0, 1, n)
    at = rng.permutation(n)
    x[at[:1000]] = 0.125
    x[at[1000:1300]] = x.min() - 1.0
    labels = (np.arange(n) & 1).astype(np.uint8)
    s = np.sort(x)[::-1]
    assert s[-1] == s[-300] != s[-301] and int((x == 0.125).sum()) >= 1000 > 3 * ROC_THREADS + 2
    want = _curve_both_ways(x, labels)
    assert len(want[0]) - 1 > ROC_THREADS * (ROC_BLOCKS - 8)                    # the second pass runs its 1024 workgroups too


def test_partition_edges_with_few_runs():
    """The same n with runs far longer than a range: 40 values, most workgroups see no run end at all."""
    n = ROC_BLOCKS * ROC_THREADS + 1
    rng = np.random.RandomState(3)
    x = rng.randint(0, 40, n) * 0.5
    labels = (rng.rand(n) < 0.3).astype(np.uint8)
    want = _curve_both_ways(x, labels)
    assert len(want[0]) - 1 == 40


# ---- 4. raw label bytes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 300, TILE + 9])
def test_raw_label_bytes(n):
    """The kernels take a label as != 0: 2, 128 and 255 are positives whatever their lowest bit."""
    rng = np.random.RandomState(n)
    labels = rng.choice(np.array([0, 1, 2, 128, 255], dtype=np.uint8), n)
    labels[rng.permutation(n)[:5]] = [0, 1, 2, 128, 255]
    assert {0, 1, 2, 128, 255} == set(labels.tolist())
    x = np.round(rng.normal(0, 1, n), 1)
    for drop in (True, False):
        _assert_curve(_raw_roc(x, labels, drop), evaluate_ref.roc_points(x, labels != 0, drop))
    for th in (0.0, 0.3, -7.0):
        want = _truth_statement(x, labels, th)
        assert _raw_truth(x, labels, th) == want and sum(want) == n


# ---- 5. the resident entries -------------------------------------------------------------------------------------------------------
def _argsort_dev(ctx, d_keys, n, descending):
    from phamers_amd import _lib, device
    d_perm = device.DeviceArray(ctx, max(n, 1), np.uint32)
    try:
        _lib.check(ctx.lib.phk_argsort_f64_dev(ctx.handle, ctypes.c_void_p(d_keys), n, 1 if descending else 0,
                                               ctypes.c_void_p(d_perm.ptr)))
        return d_perm.to_host()[:n].astype(np.int64)
    finally:
        d_perm.free()


def _resident_inputs():
    rng = np.random.RandomState(8)
    out = {}
    for name in ("rounded", "tiles_rem"):
        x, labels = evaluate_ref.stack(*evaluate_ref.cases()[name])
        at = rng.permutation(len(x))
        out[name] = (x[at], labels[at])
    assert len(out["tiles_rem"][0]) == 3 * TILE + 77
    out["one"] = (np.array([0.75]), np.array([1], dtype=np.uint8))
    return out


@pytest.mark.parametrize("name", ["rounded", "tiles_rem", "one"])
def test_resident_entries_equal_the_host_entries(name):
    from phamers_amd import _lib, device, learning
    x, labels = _resident_inputs()[name]
    n = len(x)
    ctx = _lib.get_context()
    d_scores, d_labels = device.DeviceArray.from_host(ctx, x), device.DeviceArray.from_host(ctx, labels)
    try:
        for drop in (True, False):
            got = learning.roc_points(None, None, drop, _device=(d_scores.ptr, d_labels.ptr, n))
            _assert_curve(got, learning.roc_points(x, labels, drop))
            _assert_curve(got, evaluate_ref.roc_points(x, labels, drop))
        for descending in (False, True):
            got = _argsort_dev(ctx, d_scores.ptr, n, descending)
            assert np.array_equal(got, learning.argsort_scores(x, descending=descending))
            assert np.array_equal(got, np.argsort(-(x + 0.0) if descending else x + 0.0, kind='stable'))
        assert np.array_equal(d_scores.to_host(), x) and np.array_equal(d_labels.to_host(), labels)   # the inputs are left alone
    finally:
        d_scores.free()
        d_labels.free()


def test_resident_entries_on_nothing():
    from phamers_amd import _lib, learning
    for drop in (True, False):
        fps, tps, thr, area2 = learning.roc_points(None, None, drop, _device=(0, 0, 0))
        assert fps.tolist() == [0] and tps.tolist() == [0] and thr.tolist() == [np.inf] and area2 == 0
    ctx = _lib.get_context()
    assert ctx.lib.phk_argsort_f64_dev(ctx.handle, None, 0, 0, None) == _lib.PHK_OK


# ---- 6. passes skipped between passes that run ---------------------------------------------------------------------------------------
def _argsort_both_ways(x):
    from phamers_amd import learning
    assert np.array_equal(learning.argsort_scores(x), np.argsort(x + 0.0, kind='stable'))
    assert np.array_equal(learning.argsort_scores(x, descending=True), np.argsort(-(x + 0.0), kind='stable'))


@pytest.mark.parametrize("varying", [(1, 4), (0, 2, 5), (3,), (0, 1, 2, 3, 4, 5)], ids=lambda b: "bytes" + "".join(map(str, b)))
def test_sort_passes_skipped_between_passes(varying):
    """Keys whose images differ in the chosen bytes only: two passes with skipped ones between and around them (the result
    in the first buffer of the pair), three and one (in the second), six in a row."""
    rng = np.random.RandomState(sum(varying))
    n = 3 * TILE + 5
    bits = np.full(n, 0x3ff0000000000000, dtype=np.uint64)               # 1.0; bytes 0 .. 5 are mantissa: finite, positive
    for b in varying:
        bits ^= rng.randint(0, 256, n).astype(np.uint64) << np.uint64(8 * b)
    x = bits.view(np.float64)
    assert np.isfinite(x).all() and x.min() >= 1.0 and x.max() < 2.0
    image = bits ^ np.uint64(0x8000000000000000)                         # a positive key's image: the sign bit flipped
    differ = int(np.bitwise_or.reduce(image ^ image[0]))
    assert tuple(b for b in range(8) if (differ >> (8 * b)) & 255) == varying
    assert tuple(b for b in range(8) if (int(np.bitwise_or.reduce(~image ^ ~image[0])) >> (8 * b)) & 255) == varying
    _argsort_both_ways(x)
    _curve_both_ways(x, (np.arange(n) % 3 == 1).astype(np.uint8))        # the curve writes into the pair's other buffer


# ---- 7. more than 512 tiles -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [(2 * MAX_BLOCKS + 1) * TILE - 5, 600 * TILE], ids=["1025_tiles_less_5", "600_tiles"])
def test_workgroups_of_several_tiles(n):
    """1025 tiles over 512 workgroups: two tiles each and three in the last, which holds the partial tile; 600 whole tiles:
    one or two each, no partial tile.  Small integers as keys: heavy ties, three passes."""
    tiles = -(-n // TILE)
    per_group = [tiles * (b + 1) // MAX_BLOCKS - tiles * b // MAX_BLOCKS for b in range(MAX_BLOCKS)]
    if n % TILE:
        assert set(per_group) == {2, 3} and per_group[-1] == 3
    else:
        assert set(per_group) == {1, 2} and tiles > MAX_BLOCKS
    x = np.random.RandomState(tiles).randint(0, 200, n).astype(np.float64)
    _argsort_both_ways(x)


# ---- 8. the truth table -------------------------------------------------------------------------------------------------------------
TINY = [0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 2.5e-308, 1.0, -1.0]


def test_truth_table_past_one_grid_stride():
    """3 2^20 + 77 scores: more than 256 CUs x 8 workgroups x 256 threads see in one stride."""
    from phamers_amd import learning
    n = 3 * 2 ** 20 + 77
    assert n > 256 * 8 * 256
    rng = np.random.RandomState(6)
    pos, neg = np.round(rng.normal(0.3, 1, n // 3), 2), np.round(rng.normal(0, 1, n - n // 3), 2)
    neg[-5:] = [0.3, 0.3, 9.0, -9.0, 0.29]                                       # the last elements count too
    for th in (0.3, 0.0):
        want = evaluate_ref.truth_counts(pos, neg, th)
        assert learning.truth_counts(pos, neg, th) == want and sum(want) == n
    x, labels = evaluate_ref.stack(rng.choice(TINY, n // 3), rng.choice(TINY, n - n // 3))
    for th in (-0.0, 5e-324):
        assert _raw_truth(x, labels, th) == _truth_statement(x, labels, th)


@pytest.mark.parametrize("threshold", [-0.0, 0.0, 5e-324, -5e-324, 1e-310], ids=repr)
def test_truth_table_at_signed_zero_and_subnormal_thresholds(threshold):
    from phamers_amd import learning
    rng = np.random.RandomState(7)
    pos, neg = rng.choice(TINY, 700), rng.choice(TINY, 900)
    want = evaluate_ref.truth_counts(pos, neg, threshold)
    assert learning.truth_counts(pos, neg, threshold) == want and sum(want) == 1600
    if threshold == 0.0:                                                        # either zero: -0.0 and +0.0 are >= both
        assert want[0] == int(np.sum((pos == 0) | (pos > 0))) and want == evaluate_ref.truth_counts(pos, neg, -threshold)
    assert 0 < want[0] < 700 and 0 < want[1] < 900


def test_truth_table_counts_a_nan_score_in_no_cell():
    rng = np.random.RandomState(9)
    n = 2 * TILE + 3
    x = np.round(rng.normal(0, 1, n), 1)
    labels = rng.choice(np.array([0, 1, 255], dtype=np.uint8), n)
    nan = rng.rand(n) < 0.1
    x[nan] = np.nan
    x[-1] = np.nan
    nan[-1] = True
    for th in (0.0, 0.3):
        got = _raw_truth(x, labels, th)
        assert sum(got) == n - int(nan.sum()) < n
        with np.errstate(invalid='ignore'):
            assert got == _truth_statement(x, labels, th) == _truth_statement(x[~nan], labels[~nan], th)
