"""The single-problem k-means of csrc/kmeans.hip stated in extended precision, and the inputs its tests share.

Distances, sums and means are formed in np.longdouble (64-bit mantissa on x86: every value below carries 2^-11 of a float64
rounding), and every function returns all that the device entry returns -- labels, centres, sweep count, empty clusters,
the smallest assignment gap -- so that tests/test_gpu_kmeans.py can hold phk_kmeans_lloyd and phk_kmeans to a statement
that is not another float64 computation.  oracle.kmeans_lloyd / kmeans_lloyd_seeded stay the float64 restatements;
tests/test_kmeans_host.py keeps the two in agreement on every input of the GPU file.

The inputs are dyadic (dyadic_points): integer blob centres in [0, 8) plus offsets that are multiples of 1/64 in
[-0.5, 0.5].  A difference of two such values is a multiple of 1/64 below 16, its square a multiple of 2^-12 below 2^8, and a
sum of D <= 2^10 of them needs at most 30 bits: every squared distance between data rows (and so every E-step against
seed rows, every k-means++ weight and every slice sum of the seeding walk) is exact in float64 in any summation order.
"""
import functools

import numpy as np

from oracle import oracle

LD = np.longdouble
INF = float("inf")


# ---- the statement -----------------------------------------------------------------------------------------------------------

def estep(X, centres):
    """One E-step: (labels, best, second) -- nearest centre by squared distance with ties to the lower index, the squared
    distance to it and to the runner-up (longdouble; second = inf for k = 1, = best for a tie)."""
    Xl, Cl = np.asarray(X, dtype=np.float64).astype(LD), np.asarray(centres, dtype=np.float64).astype(LD)
    n, k = Xl.shape[0], Cl.shape[0]
    d2 = np.stack([((Xl - Cl[c]) ** 2).sum(axis=1) for c in range(k)], axis=1)
    labels = np.argmin(d2, axis=1)                       # the first minimum: the lower centre index
    best = d2[np.arange(n), labels].copy()
    d2[np.arange(n), labels] = np.inf
    second = d2.min(axis=1)
    return labels.astype(np.int64), best, second


def gap_of(best, second):
    """min over points of (second - best) / second where 0 < second < inf, else inf (k = 1, or every point on two centres)."""
    ok = (second > 0) & np.isfinite(second)
    if not ok.any():
        return LD(np.inf)
    return ((second[ok] - best[ok]) / second[ok]).min()


def mstep(X, labels, centres):
    """Member means rounded to float64; an empty cluster keeps its centre.  -> (centres, sizes)"""
    X = np.asarray(X, dtype=np.float64)
    new = np.array(centres, dtype=np.float64)
    sizes = np.bincount(labels, minlength=new.shape[0])
    for c in range(new.shape[0]):
        if sizes[c]:
            new[c] = (X[labels == c].astype(LD).sum(axis=0) / LD(sizes[c])).astype(np.float64)
    return new, sizes


def lloyd_seeded(X, init, tol_abs, max_iter=300):
    """phk_kmeans_lloyd: scikit-learn's Lloyd iteration from given centres as kmeans.hip states it.  Each sweep is an E-step
    against the current centres and an M-step; the fit stops when no label changed since the previous sweep, or when the
    summed squared centre shift is <= tol_abs; in the second case, and when the sweeps run out, one more E-step follows.
    -> (labels, centres, sweeps, n_empty, min_gap, shifts): n_empty sums the empty clusters of every sweep, min_gap is
    gap_of over every E-step (the final one included), shifts holds every sweep's summed squared shift."""
    X = np.asarray(X, dtype=np.float64)
    centres = np.array(init, dtype=np.float64)
    previous = np.full(X.shape[0], -1, dtype=np.int64)
    strict, sweeps, empties, gap, shifts = False, 0, 0, LD(np.inf), []
    for it in range(max_iter):
        labels, best, second = estep(X, centres)
        gap = min(gap, gap_of(best, second))
        new, sizes = mstep(X, labels, centres)
        empties += int((sizes == 0).sum())
        shifts.append(float(((new.astype(LD) - centres.astype(LD)) ** 2).sum()))
        centres = new
        sweeps = it + 1
        if np.array_equal(labels, previous):
            strict = True
            break
        if shifts[-1] <= tol_abs:
            break
        previous = labels
    if not strict:
        labels, best, second = estep(X, centres)
        gap = min(gap, gap_of(best, second))
    return labels, centres, sweeps, empties, float(gap), shifts


def one_sweep(X, centres_in, centres_device):
    """What phk_kmeans_lloyd(max_iter = 1, tol = 0) does, evaluated at the device's own returned centres so that no
    rounding drift enters: (labels against centres_in, their means, labels against centres_device, the gap over those two
    E-steps -- longdouble)."""
    labels_in, best, second = estep(X, centres_in)
    gap = gap_of(best, second)
    means, _ = mstep(X, labels_in, centres_in)
    labels_out, best, second = estep(X, centres_device)
    return labels_in, means, labels_out, min(gap, gap_of(best, second))


def exact_gap(X, centres):
    """The float64 gap of one E-step whose squared distances are exact in float64 (dyadic rows against dyadic centres):
    the device then performs the same subtraction and the same correctly rounded division.  None when some distance is not
    a float64."""
    _, best, second = estep(X, centres)
    b, s = best.astype(np.float64), second.astype(np.float64)
    if not (np.array_equal(b.astype(LD), best) and np.array_equal(s.astype(LD), second)):
        return None
    ok = (s > 0) & np.isfinite(s)
    return float(((s[ok] - b[ok]) / s[ok]).min()) if ok.any() else INF


def kmeans_pp_lloyd(X, k, seed=10, max_iter=300):
    """phk_kmeans: k-means++ seeds (oracle.kmeans_pp_seeds: the device's slice-sum walk, operation for operation), then
    sweeps of E-step, index-ordered member means and the empty-cluster rule of kmeans.hip's header and oracle.kmeans_lloyd
    read together: every empty cluster, in index order, takes the point farthest from its own centre (the E-step's
    distance) among clusters of size > 1, ties to the lower point index; that point's distance becomes 0, the donor's centre
    and the other points' distances are not refreshed.  Stops when no label changed in the E-step and nothing was relocated,
    or after max_iter sweeps.  -> (labels, centres, sweeps, relocations, min_gap over the E-steps)"""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    centres = oracle.kmeans_pp_seeds(X, k, seed)
    labels = np.full(n, -1, dtype=np.int64)
    sweeps, relocations, gap = 0, 0, LD(np.inf)
    for it in range(max_iter):
        new, best, second = estep(X, centres)
        gap = min(gap, gap_of(best, second))
        changed = int((new != labels).sum())
        labels, own = new.copy(), best.copy()
        centres, sizes = mstep(X, labels, centres)
        for c in range(k):
            if sizes[c]:
                continue
            ok = sizes[labels] > 1
            if not ok.any():
                continue
            far = int(np.argmax(np.where(ok, own, LD(-1))))   # the first maximum: the lower point index
            sizes[labels[far]] -= 1
            labels[far] = c
            sizes[c] = 1
            own[far] = 0
            centres[c] = X[far]
            relocations += 1
            changed += 1
        sweeps = it + 1
        if changed == 0:
            break
    return labels, centres, sweeps, relocations, float(gap)


def zero_total_picks(X, centres):
    """How many k-means++ steps met an all-zero weight vector (every row already equal to a chosen centre): the pick is then
    row n - 1.  Exact on dyadic rows."""
    X = np.asarray(X, dtype=np.float64)
    mind2 = np.full(X.shape[0], np.inf)
    count = 0
    for j in range(len(centres)):
        if j and not mind2.any():
            count += 1
        mind2 = np.minimum(mind2, ((X - centres[j]) ** 2).sum(axis=1))
    return count


def centre_bound(X, labels, k):
    """Per coordinate, the distance allowed between a device centre and the statement's: (m_c + 2) * 2^-53 * max_i |X[i, d]|.
    A sequential float64 sum of m_c terms commits m_c - 1 roundings, each at most 2^-53 of a partial sum that is itself at
    most m_c max|x|; divided by m_c that is (m_c - 1) 2^-53 max|x| to first order, the division adds one rounding of a value
    <= max|x|, and the remaining two units cover the second-order terms and the statement's own rounding to float64 (its
    longdouble error is 2^-11 of this).  -> (k, D)"""
    X = np.asarray(X, dtype=np.float64)
    sizes = np.bincount(labels, minlength=k).astype(np.float64)
    return (sizes[:, None] + 2.0) * 2.0 ** -53 * np.abs(X).max(axis=0)[None, :]


def gap_bound(D):
    """|gap_device - gap_statement| for one E-step at the same float64 centres: 2 (D + 10) 2^-53, absolute.
    best and second are each a sum of at most D non-negative terms t^2 under at most D + 8 roundings: the subtraction
    counts twice in t^2, a lane's ceil(D / 64) fma steps and the 6 butterfly additions lie on a term's path, and
    2 + ceil(D / 64) + 6 <= D + 8 for every D >= 1.  All terms being non-negative, each sum carries a relative error of at
    most (D + 8) 2^-53.  With r = best / second <= 1,
    gap = 1 - r moves by at most r * 2 (D + 8) 2^-53 <= 2 (D + 8) 2^-53; the subtraction second - best and the division
    add one rounding each of a value <= 1: 2 (D + 8) 2^-53 + 2 * 2^-53 <= 2 (D + 10) 2^-53."""
    return 2.0 * (D + 10) * 2.0 ** -53


# ---- the inputs --------------------------------------------------------------------------------------------------------------

# (n, D, k): the smallest shapes that cross each boundary of the kernels -- one wave per point with lanes striding the
# columns (D = 1, 63, 65, 130), four points per workgroup (n not a multiple of 4), the 256 contiguous slices of the
# seeding's pick (n < 256, n just past 256, n = 4099 where the last slices start past n), k = 1
SHAPES = [(1, 1, 1), (5, 1, 2), (67, 3, 4), (255, 63, 7), (257, 65, 7), (1030, 130, 9), (4099, 31, 16)]
# data seed and seed-row seed of each shape (chosen so that the conditions asserted by tests/test_kmeans_host.py hold)
SEEDS = {(1, 1, 1): (1, 1), (5, 1, 2): (2, 4), (67, 3, 4): (1, 3), (255, 63, 7): (1, 3), (257, 65, 7): (1, 4),
         (1030, 130, 9): (3, 2), (4099, 31, 16): (2, 2)}
PP_SEED = 10           # learning.kmeans_seed: the seed of phk_kmeans' k-means++ draws


def dyadic_points(n, D, blobs, seed):
    """n rows around `blobs` integer centres in [0, 8)^D, offsets multiples of 1/64 in [-0.5, 0.5]."""
    rng = np.random.RandomState(seed)
    centres = rng.randint(0, 8, (blobs, D)).astype(np.float64)
    return np.ascontiguousarray(centres[rng.randint(0, blobs, n)] + rng.randint(-32, 33, (n, D)) / 64.0)


@functools.lru_cache(maxsize=None)
def shape_input(shape):
    """(X, init): the rows of a whole-fit shape and k seed rows drawn without replacement."""
    n, D, k = shape
    data_seed, row_seed = SEEDS[shape]
    X = dyadic_points(n, D, k, data_seed)
    rows = np.random.RandomState(row_seed).choice(n, k, replace=False)
    X.setflags(write=False)
    init = np.ascontiguousarray(X[rows])
    init.setflags(write=False)
    return X, init


def stopping_tolerance(shifts):
    """A tolerance at the geometric mean of two consecutive shifts of the tol = 0 fit, s_{j-1} > s_j > 0, such that every
    shift up to s_{j-1} is more than twice and s_j less than half of it: the fit with that tolerance stops at sweep j + 1,
    known in advance, whatever the device's last bits.  The latest such j short of the fit's end; None when there is none."""
    for j in range(len(shifts) - 2, 0, -1):
        if shifts[j] <= 0:
            continue
        tol = float(np.sqrt(shifts[j - 1] * shifts[j]))
        if shifts[j] * 2 < tol and all(s > 2 * tol for s in shifts[:j]):
            return tol, j + 1
    return None


@functools.lru_cache(maxsize=None)
def whole_fit(shape, tol_kind="zero", max_iter=300):
    """(tol_abs, lloyd_seeded's result) of a whole-fit shape; tol_kind: "zero", "stop" (stopping_tolerance of the zero fit;
    None when the shape has none) or "huge" (1e300)."""
    X, init = shape_input(shape)
    if tol_kind == "stop":
        found = stopping_tolerance(whole_fit(shape)[1][5])
        if found is None:
            return None
        tol = found[0]
    else:
        tol = {"zero": 0.0, "huge": 1e300}[tol_kind]
    return tol, lloyd_seeded(X, init, tol, max_iter)


@functools.lru_cache(maxsize=None)
def pp_fit(shape, k=None, max_iter=300):
    """kmeans_pp_lloyd's result on a whole-fit shape's rows (k: the shape's own unless given)."""
    return kmeans_pp_lloyd(shape_input(shape)[0], shape[2] if k is None else k, PP_SEED, max_iter)


FAR_CENTRE = 1


@functools.lru_cache(maxsize=None)
def far_centre_input():
    """The (67, 3, 4) rows with seed row FAR_CENTRE replaced by a (dyadic) point far from every row: that cluster is empty in
    every sweep."""
    X, init = shape_input((67, 3, 4))
    init = init.copy()
    init[FAR_CENTRE] = 64.0
    init.setflags(write=False)
    return X, init


# exact ties: the two points at distance 1 from both centres take centre 0
TIE_X = np.array([[0.0, 0.0], [1.0, 0.0], [2.0, 0.0], [1.0, 1.0]])
TIE_INIT = np.array([[2.0, 0.0], [0.0, 0.0]])


@functools.lru_cache(maxsize=None)
def duplicate_rows():
    """Six dyadic points five times each, permuted (n = 30)."""
    rng = np.random.RandomState(6)
    six = dyadic_points(6, 3, 6, 6)
    assert len(np.unique(six, axis=0)) == 6
    X = np.ascontiguousarray(np.repeat(six, 5, axis=0)[rng.permutation(30)])
    X.setflags(write=False)
    return X


DUPLICATE_KS = (7, 10, 30)
DUPLICATE_MAX_ITER = 5     # the relocated point returns to the lower-index duplicate centre every sweep: only the cap ends it


@functools.lru_cache(maxsize=None)
def duplicate_fit(k):
    return kmeans_pp_lloyd(duplicate_rows(), k, PP_SEED, 300 if k == 6 else DUPLICATE_MAX_ITER)


@functools.lru_cache(maxsize=None)
def tied_symmetric_set():
    """Rows on which scikit-learn's seeding (RandomState(10), k = 2) leaves points exactly between the two centres."""
    return np.array([[0.0, 0.0], [1.0, 0.0], [2.0, 0.0], [1.0, 1.0], [1.0, -1.0]])
