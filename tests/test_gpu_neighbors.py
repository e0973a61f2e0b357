"""The nearest-reference lookup on the GPU (neighbors.hip) against its host restatement (tests/neighbors_ref.py): every
comparison is array_equal on the indices and on the bit patterns of the distances, whatever route a query took -- the
certified Gram-form proposal or the exact fallback.  Every lookup here also checks the certificate's bound: the Gram-form
value of a returned row is within E of the exact chain value."""
import functools
import os

import numpy as np
import pytest

from tests import helpers, neighbors_ref as ref

pytestmark = pytest.mark.gpu

N1, M1 = 37, 300          # one partial query block; chunks of 256 + 44 rows


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(got, want):
    return np.array_equal(got[1], want[1]) and np.array_equal(bits(got[0]), bits(want[0]))


def check_bound(Q, X, got, det):
    """|Gram-form value - exact chain value| <= E for every returned row; the Gram-form value is NaN only for a row of a
    fallen-back query that the proposal had not kept.  E itself is the stated multiple of (|q| + max |x|)^2."""
    a, exact = det["approx_d2"], ref.pair_d2(Q, X, got[1])
    assert np.array_equal(bits(np.sqrt(exact)), bits(got[0]))
    assert np.all(np.isfinite(a[~det["fell_back_rows"]]))
    E = det["E"]
    assert np.all(np.abs(E - ref.bound_E(Q, X)) <= 1e-12 * E)
    err = np.where(np.isnan(a), 0.0, np.abs(a - exact))
    assert np.all(err <= E[:, None]), float((err / E[:, None]).max())
    return float((err / E[:, None]).max())


def lookup(Q, X, k, want=None, batch_rows=0):
    """learning.kneighbors with details: the result equals the restatement's, the bound holds; returns (result, details)."""
    from phamers_amd import learning
    det = {}
    got = learning.kneighbors(Q, X, k=k, _batch_rows=batch_rows, _details=det)
    want = ref.kneighbors_ref(Q, X, k) if want is None else want
    assert got[0].shape == (len(Q), k) and got[1].shape == (len(Q), k) and got[1].dtype == np.int64
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(bits(got[0]), bits(want[0]))
    assert det["queries"] == len(Q) and det["fell_back"] == int(det["fell_back_rows"].sum())
    check_bound(Q, X, got, det)
    return got, det


@functools.lru_cache(maxsize=None)
def shape_case(D):
    rng = np.random.default_rng(100 + D)
    Q, X = ref.normalised_counts(rng, N1, D), ref.normalised_counts(rng, M1, D)
    return Q, X, ref.sqdist(Q, X)


# ---- 1. shapes: the FULL path and two widths that are no multiple of the K step; every list length and its edges ---------
@pytest.mark.parametrize("k", [1, 4, 5, 12, 13, 28])
@pytest.mark.parametrize("D", [256, 100, 24])
def test_shapes(D, k):
    Q, X, d2 = shape_case(D)
    lookup(Q, X, k, want=ref.select(d2, k))


# ---- 2. past one block and one batch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [129, 300])
def test_batches_do_not_change_the_result(n):
    from phamers_amd import learning
    rng = np.random.default_rng(n)
    Q, X = ref.normalised_counts(rng, n, 100), ref.normalised_counts(rng, M1, 100)
    want = ref.kneighbors_ref(Q, X, 5)
    split, _ = lookup(Q, X, 5, want=want, batch_rows=128)
    whole = learning.kneighbors(Q, X, k=5)
    assert same(split, whole) and same(whole, want)
    assert same(learning.kneighbors(Q[:7], X, k=5), (want[0][:7], want[1][:7]))       # ... nor does N


def test_every_row_kept():
    rng = np.random.default_rng(16)
    Q, X = ref.normalised_counts(rng, 20, 100), ref.normalised_counts(rng, 16, 100)
    _, det = lookup(Q, X, 16)
    assert det["fell_back"] == 0                       # M <= KC: certified without a margin
    X[5] = X[3]
    _, det = lookup(Q, X, 16)
    assert det["fell_back"] == 0


# ---- 3. ties and duplicates on a lattice (all arithmetic exact) --------------------------------------------------------------
def test_ties_and_duplicates_are_ordered_by_index():
    rng = np.random.default_rng(3)
    D, M, u = 16, 300, 2.0 ** -8
    X = rng.integers(64, 192, (M, D)).astype(np.float64) * u
    q0 = np.full(D, 128 * u)
    spots = np.setdiff1d(np.arange(50, 290), (255, 256))
    tie = np.sort(rng.choice(spots, 40, replace=False))              # 40 rows at distance 5 u of q0, in both chunks
    assert (tie < 255).sum() > 8 and (tie > 256).sum() > 2
    for n, j in enumerate(tie):
        X[j] = q0
        if n < 32:
            X[j, n % 16] += (5 * u if n < 16 else -5 * u)
        else:
            X[j, n % 16] += 3 * u
            X[j, (n + 1) % 16] -= 4 * u
    free = np.setdiff1d(np.arange(M), tie)
    a, b, c = free[free < 250][:3]
    X[255] = X[256] = rng.integers(0, 32, D) * u                      # duplicates across the chunk cut
    q1 = X[255] + u * (np.arange(D) == 2)
    X[b] = X[c] = X[a] = rng.integers(200, 256, D) * u                # three copies of a query's nearest row
    q2 = X[a] + u * (np.arange(D) == 7)
    Q = np.vstack((q0, q1, q2, X[255], X[a]))
    for k in (5, 28):
        (dist, idx), det = lookup(Q, X, k)
        assert np.array_equal(idx[0], tie[:k]) and np.all(dist[0] == 5 * u)      # the class is cut in index order
        assert idx[1, :2].tolist() == [255, 256] and dist[1, :2].tolist() == [u, u]
        assert idx[2, :3].tolist() == sorted((a, b, c)) and idx[3, :2].tolist() == [255, 256] and dist[3, 0] == 0.0
        assert idx[4, :3].tolist() == sorted((a, b, c))
        assert det["fell_back"] > 0 and det["fell_back_rows"][0]                 # 40 equal values do not fit a list of 32


# ---- 4. cancellation -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cancellation_cases():
    rng = np.random.default_rng(4)
    X = ref.normalised_counts(rng, M1, 256)
    near = X[:20] + 1e-9 * rng.standard_normal((20, 256))
    Xo, Qo = 1000.0 + 1e-4 * rng.random((M1, 24)), 1000.0 + 1e-4 * rng.random((N1, 24))
    return X, near, Xo, Qo


def test_queries_that_are_reference_rows():
    X = cancellation_cases()[0]
    for k in (1, 5):
        (dist, idx), _ = lookup(X[:40], X, k)
        assert np.array_equal(idx[:, 0], np.arange(40)) and np.all(dist[:, 0] == 0.0)
    lookup(np.ascontiguousarray(X[250:262]), X, 13)                   # ... on both sides of the chunk cut


def test_queries_beside_reference_rows():
    X, near, _, _ = cancellation_cases()
    (dist, idx), _ = lookup(near, X, 5)
    assert np.array_equal(idx[:, 0], np.arange(20)) and np.all(dist[:, 0] < 1e-7)


def test_a_common_offset_sends_everything_to_the_fallback():
    _, _, Xo, Qo = cancellation_cases()
    for k in (4, 12, 28):
        _, det = lookup(Qo, Xo, k)
        # E = 112 * 2^-53 * (2 * 1000 sqrt(24))^2 = 1e-6, the squared distances of the noise are 4e-8: no gap survives
        assert det["fell_back"] == len(Qo)


# ---- 5. the bound, on the inputs of 1 and 4 (lookup() asserts it on every call; here: that it is not vacuous) ----------------
def test_bound_is_tight_enough_to_mean_something():
    Q, X, d2 = shape_case(256)
    (dist, idx), det = lookup(Q, X, 5, want=ref.select(d2, 5))
    assert det["fell_back"] == 0 and np.all(np.isfinite(det["approx_d2"]))
    gap = np.diff(np.sort(d2, axis=1)[:, :6] , axis=1).min(axis=1)
    assert np.all(det["E"] > 0) and np.all(det["E"] < 1e-6 * gap)                  # far below what it has to separate
    X4, near, Xo, Qo = cancellation_cases()
    for Qc, Xc in ((near, X4), (X4[:40], X4), (Qo, Xo)):
        lookup(Qc, Xc, 5)


# ---- 6. routes -------------------------------------------------------------------------------------------------------------
def test_routes_agree():
    from phamers_amd import _lib, learning
    rng = np.random.default_rng(6)
    ctx = _lib.get_context()
    pos, neg = ref.normalised_counts(rng, 140, 256), ref.normalised_counts(rng, 160, 256)
    counts = rng.integers(0, 40, (N1, 256)).astype(np.int64)
    counts[:, 3] += 1
    rows = counts.astype(np.float64) / counts.sum(axis=1, keepdims=True)
    model = _lib.Model(ctx, pos, neg)
    batch = _lib.Batch.from_counts(ctx, counts)
    try:
        for k in (3, 13):
            want = ref.kneighbors_ref(rows, np.vstack((pos, neg)), k)
            assert np.array_equal(batch.normalized().view(np.int64), rows.view(np.int64))
            assert same(batch.neighbors(model, k), want)
            assert same(model.neighbors(rows, k), want)
            assert same(learning.kneighbors(rows, np.vstack((pos, neg)), k=k), want)
    finally:
        batch.close()
        model.close()


def test_a_contig_without_counts():
    from phamers_amd import _lib, synth
    ctx = _lib.get_context()
    rng = np.random.default_rng(66)
    pos, neg = ref.normalised_counts(rng, 140, 256), ref.normalised_counts(rng, 160, 256)
    seqs = [synth.synth_contig(9, c, 600 + c) for c in range(5)]
    seqs.insert(2, "N" * 700)
    model = _lib.Model(ctx, pos, neg)
    batch = _lib.Batch.from_sequences(ctx, seqs, 4)
    try:
        with pytest.raises(ValueError, match="NaN"):
            batch.neighbors(model, 5)
        with pytest.raises(ValueError, match="NaN"):
            model.neighbors(batch.normalized(), 5)
        good = batch.select([0, 1, 3, 4, 5])
        try:
            assert same(good.neighbors(model, 5), ref.kneighbors_ref(good.normalized(), np.vstack((pos, neg)), 5))
        finally:
            good.close()
    finally:
        batch.close()
        model.close()


# ---- 7. the column mask ----------------------------------------------------------------------------------------------------
def test_column_mask():
    from phamers_amd import _lib
    ctx = _lib.get_context()
    Q, X, d2 = shape_case(256)
    rng = np.random.default_rng(7)
    mask = rng.random(M1) < 0.4
    mask[[254, 255, 257]] = True                   # neighbours of the chunk cut go, 256 stays
    mask[256] = False
    Qm = np.vstack((Q, X[255], X[256]))            # a masked row and a kept one as queries
    model = _lib.Model(ctx, X[:140], X[140:])
    try:
        plain = ref.kneighbors_ref(Qm, X, 12)
        assert same(model.neighbors(Qm, 12), plain)
        model.set_column_mask(mask)
        kept = np.flatnonzero(~mask)
        sub = ref.kneighbors_ref(Qm, X[kept], 12)
        want = ref.kneighbors_ref(Qm, X, 12, mask=mask)
        assert np.array_equal(kept[sub[1]], want[1]) and np.array_equal(bits(sub[0]), bits(want[0]))
        got = model.neighbors(Qm, 12)
        assert same(got, want) and not mask[got[1]].any() and got[1][-1, 0] == 256 and got[1][-2, 0] != 255
        few = np.ones(M1, bool)
        few[[3, 255, 256, 299]] = False
        few[140:150] = False                       # 14 rows left, some in each class
        model.set_column_mask(few)
        assert same(model.neighbors(Qm, 13), ref.kneighbors_ref(Qm, X, 13, mask=few))     # every kept row fits the list
        assert same(model.neighbors(Qm, 14), ref.kneighbors_ref(Qm, X, 14, mask=few))
        with pytest.raises(ValueError, match="unmasked"):
            model.neighbors(Qm, 15)
        model.set_column_mask(None)
        assert same(model.neighbors(Qm, 12), plain)
    finally:
        model.close()


# ---- 8. real data ----------------------------------------------------------------------------------------------------------
def test_real_data():
    from phamers_amd import learning
    X, _, _ = ref.reference_rows(helpers.GOLDEN)
    Q = np.vstack((helpers.load_npz("scoring_k4.npz")["q"], X[:300]))
    want = ref.kneighbors_screened(Q, X, 5)
    det = {}
    got = learning.kneighbors(Q, X, k=5, _details=det)
    assert same(got, want)
    worst = check_bound(Q, X, got, det)
    print("fallback %d of %d; largest |approx - exact| / E = %.3g" % (det["fell_back"], len(Q), worst))
    # a condition, not a measurement: the bound is some 30 times the Gram form's observed error and the rows' gaps are
    # far wider; a higher share means the bound or the list is wrong
    assert det["fell_back"] <= 0.01 * len(Q)


# ---- 9. the command line ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strands", [[], ["--both_strands"]])
def test_command_line(tmp_path, strands):
    from phamers_amd import fileIO, kmer, learning, phamer, synth, transform_kmers
    f = helpers.load_npz("ref_features.npz")
    data = tmp_path / "data" / "reference_features"
    data.mkdir(parents=True)
    fileIO.save_counts(f["pos_counts"][:400], f["pos_ids"][:400], str(data / "positive_features.csv"))
    fileIO.save_counts(f["neg_counts"][:400], f["neg_ids"][:400], str(data / "negative_features.csv"))
    indir = tmp_path / "in"
    indir.mkdir()
    seqs = [synth.synth_contig(12, c, 5000 + 17 * c) for c in range(12)]
    ids = ["SuperContig_%d_length_%d_ID_%d" % (c, len(s), c) for c, s in enumerate(seqs)]
    with open(indir / "contigs.fasta", "w") as fa:
        for name, s in zip(ids, seqs):
            fa.write(">%s\n%s\n" % (name, "\n".join(s[i:i + 70] for i in range(0, len(s), 70))))
    argv = ["-in", str(indir), "-data", str(tmp_path / "data")] + strands
    out = indir / "phamer_output"
    phamer.main(argv)
    plain = (out / "phamer_scores.csv").read_bytes()
    assert not (out / "phamer_neighbors.csv").exists()
    scorer = phamer.main(argv + ["--neighbors", "3"])
    assert (out / "phamer_scores.csv").read_bytes() == plain
    contigs = [str(i) for i in scorer.data_ids]                  # (the parsed ids, as phamer_scores.csv lists them)
    assert len(contigs) == 12 and contigs == list(fileIO.read_phamer_output(str(out / "phamer_scores.csv")))
    rows = fileIO.read_phamer_neighbors(str(out / "phamer_neighbors.csv"))
    both = bool(strands)
    pos, neg = (transform_kmers.fold_strands(f[n][:400].astype(np.int64)) if both else f[n][:400].astype(np.int64) for n in ("pos_counts", "neg_counts"))
    X = np.vstack((pos, neg)).astype(np.float64)
    X /= X.sum(axis=1, keepdims=True)
    q = kmer.count(seqs, 4, both_strands=both).astype(np.float64)
    dist, idx = learning.kneighbors(q / q.sum(axis=1, keepdims=True), X, k=3)
    ref_ids = np.concatenate((f["pos_ids"][:400], f["neg_ids"][:400]))
    want = [(contigs[a], r + 1, str(ref_ids[idx[a, r]]), "positive" if idx[a, r] < 400 else "negative", float(dist[a, r]))
            for a in range(12) for r in range(3)]
    assert rows == want
    text = (out / "phamer_neighbors.csv").read_text()
    assert text.startswith("# PhaMers nearest reference file\n") and "# neighbors:\t3\n" in text
