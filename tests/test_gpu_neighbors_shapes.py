"""The nearest-reference lookup (neighbors.hip) past the shapes of tests/test_gpu_neighbors.py: row counts on every chunk,
step and half-step edge and with chunks shorter than the candidate list, many chunks, query counts around the query block
at every list length, the fallback in batches after the first and in more than one round, masks that empty a chunk or a
step, widths from one column to 4096, mixed signs and zeros, power-of-two scalings, and the shared workspaces.

Every comparison is array_equal on the indices and on the int64 view of the distances against tests/neighbors_ref.py, and
every call with details also checks |Gram-form value - chain value| <= E (lookup() / check_bound() of the sibling file).
Which route a query takes is asserted too, from two predicates on the reference alone (neighbors_ref.must_certify /
must_fall_back: derived from the certificate, not measured): each test first asserts on the host that its inputs decide
the route, then looks at the device.

Left out: magnitudes at which a square overflows or underflows (the scalings stay at 2^+-200, where the chain, the Gram
form and the host's fma emulation are all exact images of the unscaled run)."""
import functools

import numpy as np
import pytest

from tests import neighbors_ref as ref
from tests.test_gpu_neighbors import bits, lookup, same

pytestmark = pytest.mark.gpu

KS = (4, 12, 28)                   # list lengths 8, 16, 32


def list_length(k):
    return 8 if k <= 4 else (16 if k <= 12 else 32)


def routes(d2, E, k, expect):
    """The two predicates on the reference.  ``expect`` (N,) bool or None: the queries that fall back -- then the inputs
    have to decide every query that way; None: whatever the predicates decide."""
    KC = list_length(k)
    yes, no = ref.must_certify(d2, E, k, KC), ref.must_fall_back(d2, k, KC)
    assert not (yes & no).any()
    if expect is not None:
        assert np.array_equal(no, expect) and np.array_equal(yes, ~expect), (np.flatnonzero(no != expect), np.flatnonzero(yes == expect))
    return yes, no


def routed(Q, X, k, d2, expect=None, batch_rows=0, want=None):
    """lookup() against the selection from d2, with the route of every decided query asserted.  Returns (result, details)."""
    if isinstance(expect, bool):
        expect = np.full(len(Q), expect)
    yes, no = routes(d2, ref.bound_E(Q, X), k, expect)                    # ... before the device is asked
    got, det = lookup(Q, X, k, want=ref.select(d2, k) if want is None else want, batch_rows=batch_rows)
    fb = det["fell_back_rows"]
    assert not fb[yes].any() and fb[no].all(), (np.flatnonzero(fb & yes), np.flatnonzero(~fb & no))
    if expect is not None:
        assert np.array_equal(fb, expect) and det["fell_back"] == int(expect.sum())
    return got, det


def tie_class(centre, u):
    """40 distinct rows at squared distance 25 u^2 of ``centre`` (D >= 16): +-5 u on one coordinate, or (3 u, -4 u) on two."""
    rows = np.tile(centre, (40, 1))
    for n in range(40):
        if n < 32:
            rows[n, n % 16] += 5 * u if n < 16 else -5 * u
        else:
            rows[n, n % 16] += 3 * u
            rows[n, (n + 1) % 16] -= 4 * u
    return rows


# ---- A. row edges of the proposal ------------------------------------------------------------------------------------------
ROW_EDGES = (29, 31, 32, 33, 63, 64, 65, 255, 256, 257, 288, 289, 512, 513, 1027)


@functools.lru_cache(maxsize=None)
def row_case(D):
    rng = np.random.default_rng(1000 + D)
    Q, X = ref.normalised_counts(rng, 130, D), ref.normalised_counts(rng, max(ROW_EDGES), D)
    return Q, X, ref.sqdist(Q, X)


@pytest.mark.parametrize("M", ROW_EDGES)
@pytest.mark.parametrize("D", [24, 32])
def test_row_edges(D, M):
    """One query block and two queries against M rows: the chunk (256), step (64) and half-step (32) edges and one past
    them; at 257, 513 and 1027 the last chunk has 1 or 3 rows and pads every list.  Nothing falls back."""
    Q, X, d2 = row_case(D)
    for k in KS:
        if k <= M:
            routed(Q, np.ascontiguousarray(X[:M]), k, d2[:, :M], expect=False)


# ---- B. many chunks ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chunks_case():
    rng = np.random.default_rng(2000)
    M, D, N = 40 * 256 + 7, 16, 20
    Q, X = ref.normalised_counts(rng, N, D), ref.normalised_counts(rng, M, D)
    spread = [17, M - 7] + [256 * c + int(rng.integers(0, 256)) for c in range(1, 27)]           # one row per chunk
    tail = list(range(M - 6, M - 1)) + list(range(39 * 256 + 100, 39 * 256 + 123))                # last chunk, then the one before
    step = 5 * 256 + 128
    upper = [step + 32] + list(range(step + 37, step + 64))                                      # the upper half of one step
    planted = {0: spread, 1: tail, 2: upper}
    assert len(set(spread + tail + upper)) == 3 * 28 and 0 not in spread + tail + upper and M - 1 not in spread + tail + upper
    for q, rows in planted.items():
        for n, j in enumerate(rows):                                       # the n-th nearest of query q: (n + 1) 2e-4 away
            X[j] = Q[q]
            X[j, n % D] += (n + 1) * 2e-4
    Q[3], Q[4] = X[0], X[M - 1]
    return Q, X, ref.sqdist(Q, X), planted


@pytest.mark.parametrize("k", KS)
def test_many_chunks(k):
    Q, X, d2, planted = chunks_case()
    want = ref.select(d2, k)
    for q, rows in planted.items():                                        # the neighbours are where they were planted
        assert want[1][q].tolist() == rows[:k]
    M = len(X)
    assert want[1][3, 0] == 0 and want[1][4, 0] == M - 1 and want[0][3, 0] == 0.0 and want[0][4, 0] == 0.0
    assert {j // 256 for j in planted[0][:k]} >= {0, 40} and len({j // 256 for j in planted[0][:k]}) == k
    routed(Q, X, k, d2, expect=False, want=want)


# ---- C. query edges at every list length -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def query_case():
    rng = np.random.default_rng(3000)
    Q, X = ref.normalised_counts(rng, 257, 24), ref.normalised_counts(rng, 300, 24)
    return Q, X, ref.sqdist(Q, X)


@pytest.mark.parametrize("k", [4, 28])
@pytest.mark.parametrize("n", [1, 127, 128, 129, 256, 257])
def test_query_edges(n, k):
    """Around one and two query blocks; the refinement packs 32 or 8 queries per workgroup.  Whole and in batches of 128."""
    from phamers_amd import learning
    Q, X, d2 = query_case()
    q, want = np.ascontiguousarray(Q[:n]), ref.select(d2[:n], k)
    whole, _ = routed(q, X, k, d2[:n], expect=False, want=want)
    split, _ = routed(q, X, k, d2[:n], expect=False, want=want, batch_rows=128)
    assert same(whole, split) and same(learning.kneighbors(q, X, k=k), want)
    if n == 257:
        assert same(learning.kneighbors(Q[:7], X, k=k), (want[0][:7], want[1][:7]))


# ---- D. the fallback in every batch ----------------------------------------------------------------------------------------------
PLANTED = (0, 5, 64, 127, 128, 200, 255, 256, 270, 299)


@functools.lru_cache(maxsize=None)
def fallback_case():
    rng = np.random.default_rng(4000)
    D, M, N, u = 16, 300, 300, 2.0 ** -8
    X = rng.integers(64, 192, (M, D)).astype(np.float64) * u
    centres = np.full(D, 128 * u), np.full(D, 100 * u)
    spots = rng.permutation(M)                                             # both classes in both chunks
    ties = np.sort(spots[:40]), np.sort(spots[40:80])
    for c, t in zip(centres, ties):
        X[t] = tie_class(c, u)
        assert (t < 256).sum() > 8 and (t >= 256).sum() > 1
    Q = (64 + 128 * rng.random((N, D))) * u                                # off the lattice: no two rows equally far
    for n, q in enumerate(PLANTED):
        Q[q] = centres[n % 2]
    expect = np.zeros(N, bool)
    expect[list(PLANTED)] = True
    d2 = ref.sqdist(Q, X)
    assert np.array_equal(d2[list(PLANTED)], ref.lattice_sqdist(Q[list(PLANTED)], X))
    return Q, X, d2, expect, ties, u


@pytest.mark.parametrize("k", [4, 28])
def test_fallback_in_every_batch(k):
    """Three batches of 128, 128 and 44 queries; each holds lattice centres with 40 rows at their k-th place, at its first
    and last query and inside: the batch-local list of fallen-back queries, the offset of their output rows and the
    counter's reset all run past the first batch.  Every other query is certified."""
    Q, X, d2, expect, ties, u = fallback_case()
    want = ref.select(d2, k)
    for n, q in enumerate(PLANTED):
        assert np.array_equal(want[1][q], ties[n % 2][:k]) and np.all(want[0][q] == 5 * u)         # cut in index order
    split, det = routed(Q, X, k, d2, expect=expect, want=want, batch_rows=128)
    assert det["fell_back"] == len(PLANTED)
    whole, det = routed(Q, X, k, d2, expect=expect, want=want)
    assert same(split, whole) and det["fell_back"] == len(PLANTED)


# ---- E. more than one fallback round ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rounds_case():
    """A lattice in the plane: 2^15 + 3 rows on 256 points, 1100 queries on a grid twice as fine.  The fallback takes
    2^28 / (8 M) = 1023 queries per round, so 1100 > 2^25 / M of them make two rounds."""
    rng = np.random.default_rng(5001)
    M, N = 2 ** 15 + 3, 1100
    X = rng.integers(0, 16, (M, 2)).astype(np.float64) * 2.0 ** -6
    Q = rng.integers(0, 32, (N, 2)).astype(np.float64) * 2.0 ** -7
    assert (256 << 20) // (8 * M) == 1023 < N
    d2 = ref.lattice_sqdist(Q, X)
    assert np.array_equal(d2[:3, :2000], ref.sqdist(Q[:3], X[:2000]))
    E = ref.bound_E(Q, X)
    for k in (4, 28):
        routes(d2, E, k, np.ones(N, bool))                                 # every query has to fall back ...
        assert (d2 <= ref._order_statistic(d2, k)[:, None]).sum(axis=1).min() >= 100       # ... with room: lists hold 32
    return Q, X, ref.select_by_partition(d2, 28)


@pytest.mark.parametrize("k", [4, 28])
def test_fallback_rounds(k):
    """Every query falls back (asserted on the reference in rounds_case): rounds of 1023 and 77 queries, a select over 129
    strides of 256 rows with classes of 100 and more equal values."""
    Q, X, want = rounds_case()
    got, det = lookup(Q, X, k, want=(want[0][:, :k], want[1][:, :k]))      # (the first k of the first 28)
    assert det["fell_back"] == len(Q) and det["fell_back_rows"].all()


# ---- F. the column mask ------------------------------------------------------------------------------------------------------------
def masked_lookup(ctx, model, Q, X, k, mask, d2, expect):
    """Model.neighbors under ``mask`` against the masked reference; the route from the predicates on the masked reference
    (before the device), the fallback count from the context's statistics."""
    d2 = d2.copy()
    if mask is not None:
        d2[:, mask] = np.inf
    expect = np.full(len(Q), expect) if isinstance(expect, bool) else expect
    routes(d2, ref.bound_E(Q, X), k, expect)                               # (the bound's max |x| runs over masked rows too)
    want = ref.select(d2, k)
    ctx.neighbors_stats()
    got = model.neighbors(Q, k)
    stats = ctx.neighbors_stats()
    assert np.array_equal(got[1], want[1]) and np.array_equal(bits(got[0]), bits(want[0]))
    assert mask is None or not mask[got[1]].any()
    assert stats == (len(Q), int(expect.sum())), stats
    return got


@functools.lru_cache(maxsize=None)
def mask_case():
    rng = np.random.default_rng(6000)
    M, D = 1027, 32
    Q, X = ref.normalised_counts(rng, 40, D), ref.normalised_counts(rng, M, D)
    X[300], X[301], X[600] = Q[0], Q[1], Q[1]              # copies of queries in the masked chunk and the masked step ...
    X[700], X[20] = Q[0], Q[1]                             # ... and copies that stay
    X[1025] = Q[2]
    Q[3], Q[4] = X[400], X[1024]                           # a masked row and the last chunk's only kept row as queries
    return Q, X, ref.sqdist(Q, X)


def test_mask_empties_a_chunk_and_a_step():
    from phamers_amd import _lib
    ctx = _lib.get_context()
    Q, X, d2 = mask_case()
    mask = np.zeros(len(X), bool)
    mask[256:512] = True                                   # all of chunk 1
    mask[512 + 64:512 + 128] = True                        # one step of chunk 2
    mask[1025:] = True                                     # all but one row of the last chunk
    model = _lib.Model(ctx, X[:500], X[500:])
    try:
        for k in KS:
            plain = masked_lookup(ctx, model, Q, X, k, None, d2, False)
            assert plain[1][0, :2].tolist() == [300, 700] and plain[1][1, :3].tolist() == [20, 301, 600]
            model.set_column_mask(mask)
            got = masked_lookup(ctx, model, Q, X, k, mask, d2, False)
            # no masked copy comes back, the kept copy comes first
            assert got[1][0, 0] == 700 and got[1][1, 0] == 20 and got[0][0, 0] == 0.0 and got[0][1, 0] == 0.0
            assert got[0][2, 0] > 0.0 and got[0][3, 0] > 0.0 and got[1][4, 0] == 1024
            model.set_column_mask(None)                    # ... and off again
            assert same(masked_lookup(ctx, model, Q, X, k, None, d2, False), plain)
    finally:
        model.close()


def test_mask_leaves_fewer_rows_than_a_list():
    """Ten rows left in chunks 0, 2 and 4: every chunk's list is padded.  k = 10: every kept row fits the list of 16;
    k = 4: a list of 8 for ten rows, certified by the gap."""
    from phamers_amd import _lib
    ctx = _lib.get_context()
    Q, X, d2 = mask_case()
    kept = [3, 100, 255, 512, 575, 700, 767, 1024, 1025, 1026]
    mask = np.ones(len(X), bool)
    mask[kept] = False
    model = _lib.Model(ctx, X[:500], X[500:])
    try:
        model.set_column_mask(mask)
        got = masked_lookup(ctx, model, Q, X, 10, mask, d2, False)
        assert np.array_equal(np.sort(got[1], axis=1), np.tile(kept, (len(Q), 1)))
        masked_lookup(ctx, model, Q, X, 4, mask, d2, False)
        with pytest.raises(ValueError, match="unmasked"):
            model.neighbors(Q, 11)
    finally:
        model.close()


@functools.lru_cache(maxsize=None)
def mask_ties_case():
    rng = np.random.default_rng(6500)
    M, D, N, u = 1027, 32, 30, 2.0 ** -8
    X = rng.integers(64, 192, (M, D)).astype(np.float64) * u
    a, b = np.full(D, 128 * u), rng.integers(90, 110, D) * u              # (b uneven: a's class is not a class seen from b)
    spots = rng.permutation(np.setdiff1d(np.arange(M), (255, 256, 1026)))
    ta, tb, copies = np.sort(spots[:40]), np.sort(spots[40:80]), spots[80:87]
    X[ta], X[tb] = tie_class(a, u), tie_class(b, u)
    X[copies[:2]], X[copies[2:]] = a, b                    # exact copies of both centres: all masked
    X[255] = X[256] = X[1026] = a
    mask = np.zeros(M, bool)
    mask[copies] = mask[[255, 256, 1026]] = True
    mask[ta[[0, 13, 27, 39]]] = True                       # 36 of a's 40 rows stay: more than any list
    mask[tb[4:]] = True                                    # 4 of b's stay
    Q = (64 + 128 * rng.random((N, D))) * u
    A, B = [0, 7, 29], [1, 15]
    Q[A], Q[B] = a, b
    return Q, X, ref.sqdist(Q, X), mask, A, B, (ta, tb), u


@pytest.mark.parametrize("k", [4, 28])
def test_mask_and_fallback(k):
    """Lattice centres under a mask: centre a keeps 36 equally distant rows (more than a list: falls back), centre b keeps 4
    (certified), the exact copies of both are masked.  Without the mask the copies come first and both classes of 40 count."""
    from phamers_amd import _lib
    ctx = _lib.get_context()
    Q, X, d2, mask, A, B, (ta, tb), u = mask_ties_case()
    expect = np.zeros(len(Q), bool)
    expect[A] = True
    model = _lib.Model(ctx, X[:500], X[500:])
    try:
        model.set_column_mask(mask)
        got = masked_lookup(ctx, model, Q, X, k, mask, d2, expect)
        for q in A:
            assert np.array_equal(got[1][q], ta[~mask[ta]][:k]) and np.all(got[0][q] == 5 * u)
        for q in B:
            assert np.array_equal(got[1][q, :4], tb[:4]) and np.all(got[0][q, :4] == 5 * u)
        model.set_column_mask(None)
        plain = np.zeros(len(Q), bool)                     # 5 copies, then 40 rows: the k-th place is in the class at k = 28 only
        plain[A + B] = k > 5
        got = masked_lookup(ctx, model, Q, X, k, None, d2, plain)
        assert np.all(got[0][A + B, :4] == 0.0) and np.all(got[0][A + B, 5:] == 5 * u)
    finally:
        model.close()


# ---- G. width ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def width_case(D):
    rng = np.random.default_rng(7000 + D)
    N = 37 if D < 1024 else 9
    if D <= 2:                                             # (normalised counts are all 1.0 at D = 1 and a segment at D = 2)
        Q, X = rng.random((N, D)), rng.random((300, D))
    else:
        Q, X = ref.normalised_counts(rng, N, D), ref.normalised_counts(rng, 300, D)
    return Q, X, ref.sqdist(Q, X)


@pytest.mark.parametrize("D", [1, 2, 7, 8, 9, 31, 33, 63, 65, 1024, 4096])
def test_widths(D):
    """Below one lane slot of 8 columns, around one and two K steps of 32, and wide: E grows with D, the Gram form's error
    has to stay below it.  Prints the largest |Gram-form value - chain value| / E."""
    Q, X, d2 = width_case(D)
    worst = 0.0
    for k in KS:
        got, det = routed(Q, X, k, d2, expect=False)                       # (asserts the bound; the ratio again from d2)
        err = np.abs(det["approx_d2"] - np.take_along_axis(d2, got[1], axis=1)) / det["E"][:, None]
        worst = max(worst, float(err.max()))
    print("D = %d: largest |approx - exact| / E = %.3g" % (D, worst))


# ---- H. values -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def values_case():
    rng = np.random.default_rng(8000)
    Q, X = rng.standard_normal((40, 24)), rng.standard_normal((300, 24))
    Q[0] = 0.0                                             # an all-zero query
    X[17] = X[200] = 0.0                                   # two all-zero rows: equally far from every query
    Q[1] = -X[5]                                           # the negative of a row
    Q[2] = X[17]
    return Q, X, ref.sqdist(Q, X)


@pytest.mark.parametrize("k", [5, 28])
def test_mixed_signs_zeros_and_scaling(k):
    Q, X, d2 = values_case()
    want = ref.select(d2, k)
    assert want[1][0, :2].tolist() == [17, 200] and want[0][0, 0] == 0.0 and want[0][2, 1] == 0.0
    for q in range(len(Q)):                                # wherever both zero rows are returned they are adjacent, 17 first
        at = np.flatnonzero(np.isin(want[1][q], (17, 200)))
        assert len(at) < 2 or (want[1][q, at].tolist() == [17, 200] and at[1] == at[0] + 1)
    assert d2[1, 5] == 4.0 * d2[0, 5] and 5 not in want[1][1]              # (-x) - x = -2 x: far from its own row
    yes, no = routes(d2, ref.bound_E(Q, X), k, None)
    assert yes.all()                                                       # (a class of two never spans places k .. KC)
    (dist, idx), det = routed(Q, X, k, d2, expect=False, want=want)
    for s in (2.0 ** 200, 2.0 ** -200):                                    # exact: every intermediate scales by s or s^2
        _, det_s = lookup(Q * s, X * s, k, want=(dist * s, idx))
        assert np.array_equal(bits(det_s["E"]), bits(det["E"] * (s * s)))
        decided = yes | no
        assert np.array_equal(det_s["fell_back_rows"][decided], det["fell_back_rows"][decided])


# ---- I. state ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def state_case():
    rng = np.random.default_rng(9000)
    Q, X = ref.normalised_counts(rng, 257, 32), ref.normalised_counts(rng, 1027, 32)
    q, x = ref.normalised_counts(rng, 3, 24), ref.normalised_counts(rng, 29, 24)
    return Q, X, ref.sqdist(Q, X), q, x, ref.sqdist(q, x)


def test_calls_do_not_leak_into_each_other():
    """A large call with lists of 32, a small one with lists of 8, a density call (the same partials workspace) and the
    large call again; then the same call with and without details."""
    from phamers_amd import learning
    Q, X, d2, q, x, e2 = state_case()
    rng = np.random.default_rng(9001)
    kq, kx = ref.normalised_counts(rng, 150, 64), ref.normalised_counts(rng, 700, 64)
    density = learning.log_density(kq, kx, 0.05)
    first, _ = routed(Q, X, 28, d2, expect=False)
    routed(q, x, 4, e2, expect=False)
    again = learning.log_density(kq, kx, 0.05)
    assert np.array_equal(bits(again), bits(density)) and np.all(np.isfinite(density))
    last, _ = routed(Q, X, 28, d2, expect=False)
    assert same(first, last)
    assert same(learning.kneighbors(Q, X, k=28), first)                   # ... and without details
    routed(q, x, 4, e2, expect=False, batch_rows=128)
    assert same(learning.kneighbors(q, x, k=4), ref.select(e2, 4))
