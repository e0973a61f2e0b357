"""GPU: the cross-validation state of one resident model (phk_model_set_centroids, phk_model_set_column_mask,
phk_model_set_bandwidths, phk_model_fit_svm) in any call order.  After every operation of one seeded sequence, each
scoring path and entry point of the resident model must give the scores of a FRESH model built from the unmasked rows
with the current centroids, bandwidths and svm fit, and those of the float64 restatements of those rows.

Bars (the suite's own): knn bit-equal; kmeans / combo within 1e-12 relative of the fresh model and 1e-6 of the oracle;
density within 1e-11 x max(1, |want|) (tests/density_ref.py); svm bit-equal to a fresh fit on the rows of the last
successful fit (the fit is a snapshot: a later mask does not change it).

The queries that matter are the held-out rows themselves and count vectors drawn from them: a masked train row that
leaks back into the search is their nearest neighbour."""
import numpy as np
import pytest

from tests import density_ref, helpers

pytestmark = pytest.mark.gpu
RTOL = 1e-6
F64 = 1e-11
ALL = ("knn", "kmeans", "combo", "density", "svm")
KNS = (1, 3, 5)          # kn = 5 is past the MFMA paths' candidate lists: the float64 path with phk_mask_dist_kernel


def _i8_sweeps(prof):
    return prof.get("phk_knn_i8_general_kernel", (0.0, 0))[1]


def _ref_matrices():
    from oracle import oracle
    ref = helpers.load_npz("ref_features.npz")
    return (oracle.normalize_counts(ref["pos_counts"].astype(np.int64)),
            oracle.normalize_counts(ref["neg_counts"].astype(np.int64)))


def _data(tag):
    """(pos, neg, cpos, cneg, host queries, count queries or None, k)"""
    if tag == "k4":
        g = helpers.load_npz("scoring_k4.npz")
        pos, neg = _ref_matrices()
        return pos, neg, g["cpos_full"], g["cneg_full"], np.vstack((g["q"], g["adv_q"])), g["q_counts"], 4
    g = helpers.load_npz("scoring_highdim.npz")
    return g["pos_" + tag], g["neg_" + tag], g["cpos_" + tag], g["cneg_" + tag], g["q_" + tag], None, int(tag[1])


class Oracle(object):
    """float64 restatements of every method over the current unmasked rows (top-5 neighbours once per state)."""

    def __init__(self, Q, pos, neg, cp, cn, bw):
        from oracle import oracle
        train = np.vstack((pos, neg))
        labels = np.append(np.ones(len(pos)), np.zeros(len(neg)))
        _, nbr, _ = oracle.knn(Q, train, labels, k=min(5, len(train)), return_neighbors=True)
        self.votes = np.cumsum(labels[nbr], axis=1)
        self.kmeans = oracle.centroid_score_points_fast(Q, cp, cn)
        self.density = density_ref.density_scores(Q, pos, neg, *bw) if len(pos) and len(neg) else None

    def knn(self, kn):
        return 2.0 * ((self.votes[:, kn - 1] * 2 > kn).astype(float) - 0.5)


class FoldState(object):
    """One resident model per kn, driven through the same operations, checked against fresh models and the oracle."""

    def __init__(self, ctx, tag, seed):
        from phamers_amd import _lib, device
        self.ctx, self.lib, self.device = ctx, _lib, device
        self.pos, self.neg, self.cp0, self.cn0, self.q, q_counts, self.k = _data(tag)
        self.D = self.pos.shape[1]
        self.M = len(self.pos) + len(self.neg)
        self.rng = np.random.default_rng(seed)
        self.q_counts = q_counts if q_counts is not None else np.zeros((0, self.D), np.uint32)
        self.models = {kn: _lib.Model(ctx, self.pos, self.neg, self.cp0, self.cn0, kn) for kn in KNS}
        self.kns = KNS
        self.state = dict(mask=None, cents=(self.cp0, self.cn0), bw=(0.005, 0.01), svm=None)
        self.held = np.zeros(self.M, bool)            # the rows whose count queries are drawn (the last mask's held-out rows)
        self.paths = [{}, {"force_exact": ("1", "0")}] + ([{"proposal": ("hi", "")}] if self.D != 256 else [])
        # synthetic contigs for phk_count_score_dev (counts made on the device, then scored under the mask)
        n, L = {4: (48, 5000), 5: (32, 20000), 6: (16, 40000)}[self.k]
        self.syn_n, self.syn_T = n, n * L
        self.d_packed = device.DeviceArray(ctx, device.packed_words(self.syn_T), np.uint32)
        self.d_off = device.DeviceArray(ctx, n + 1, np.uint64)
        device.synth_packed(ctx, 5 + self.k, 0, n, L, self.d_packed, self.d_off)
        self.svm_fresh = None

    def close(self):
        for m in self.models.values():
            m.close()
        if self.svm_fresh is not None:
            self.svm_fresh.close()

    # ---- the operations -------------------------------------------------------------------------------------
    def unmasked(self, mask=None):
        mask = self.state["mask"] if mask is None else mask
        if mask is None:
            return self.pos, self.neg
        return self.pos[~mask[:len(self.pos)]], self.neg[~mask[len(self.pos):]]

    def fold_centroids(self, mask, hot=False):
        """Per-class strided means of the unmasked rows, as many as at creation; hot: the first positive centroid is
        the one-hot row of a homopolymer contig, far from the centring vector (its bias term dwarfs the others)."""
        p, n = self.unmasked(mask)
        cp = np.stack([p[i::len(self.cp0)].mean(axis=0) for i in range(len(self.cp0))])
        cn = np.stack([n[i::len(self.cn0)].mean(axis=0) for i in range(len(self.cn0))])
        if hot:
            cp[0] = 0.0
            cp[0, 0] = 1.0
        return cp, cn

    def random_mask(self, frac):
        return self.rng.random(self.M) < frac

    def set_centroids(self, cents):
        for m in self.models.values():
            m.set_centroids(*cents)
        self.state["cents"] = cents

    def set_mask(self, mask):
        for m in self.models.values():
            m.set_column_mask(mask)
        self.state["mask"] = mask
        if mask is not None:
            self.held = mask.copy()

    def set_bandwidths(self, hp, hn):
        for m in self.models.values():
            m.set_bandwidths(hp, hn)
        self.state["bw"] = (hp, hn)

    def fit_svm(self):
        p, n = self.unmasked()
        if len(p) == 0 or len(n) == 0:
            for m in self.models.values():
                with pytest.raises(ValueError):
                    m.fit_svm()
            return                                      # (the previous fit stays: checked by the next check())
        gammas = {m.fit_svm() for m in self.models.values()}
        if self.svm_fresh is not None:
            self.svm_fresh.close()
        self.svm_fresh = self.lib.Model(self.ctx, p, n, k_neighbors=1)
        assert gammas == {self.svm_fresh.fit_svm()}
        self.state["svm"] = True

    # ---- the check ------------------------------------------------------------------------------------------
    def queries(self):
        """host rows: the fixed queries + held-out rows; counts: the fixed count queries + ~1e6-base draws from held-out rows"""
        idx = np.flatnonzero(self.held)
        pick = idx[np.linspace(0, len(idx) - 1, min(len(idx), 40)).astype(int)] if len(idx) else idx
        train = np.vstack((self.pos, self.neg))
        Q = np.vstack((self.q, train[pick]))
        draws = [self.rng.multinomial(1000000 + 7919 * i, train[r] / train[r].sum()) for i, r in enumerate(pick[::2])]
        C = np.vstack([self.q_counts] + draws).astype(np.uint32) if draws or len(self.q_counts) else None
        return Q, C

    def run(self, model, Q, C, method):
        """{entry point: scores} for one model and method; a refused call gives its PhkError."""
        lib, device, ctx = self.lib, self.device, self.ctx
        out = {}

        def guard(name, fn):
            try:
                out[name] = fn()
            except lib.PhkError as e:
                out[name] = e

        guard("host", lambda: model.score(Q, method))
        if C is not None:
            d_c = device.DeviceArray.from_host(ctx, C)
            d_s = device.DeviceArray(ctx, len(C), np.float64)
            d_st = device.DeviceArray(ctx, 1, np.uint32)

            def counts():
                device.score_counts(ctx, model, d_c, len(C), method, d_s, d_st)
                assert d_st.to_host()[0] == 0
                return d_s.to_host()
            guard("counts", counts)
            b = lib.Batch.from_counts(ctx, C)
            assert b is not None
            guard("batch", lambda: b.score(model, method))
            b.close()
        d_counts = device.DeviceArray(ctx, (self.syn_n, self.D), np.uint32)
        d_s = device.DeviceArray(ctx, self.syn_n, np.float64)

        def fused():
            device.count_score(ctx, model, self.d_packed, None, self.syn_T, self.d_off, self.syn_n, self.k, method, d_counts, d_s)
            got = d_s.to_host()
            d_s2 = device.DeviceArray(ctx, self.syn_n, np.float64)
            device.score_counts(ctx, model, d_counts, self.syn_n, method, d_s2)
            assert np.array_equal(got, d_s2.to_host()), (method, "count_score != score_counts on its own counts")
            return got
        guard("fused", fused)
        if "fused" in out and not isinstance(out["fused"], Exception):
            self.syn_counts = d_counts.to_host()
        return out

    def check(self, what, QC=None):
        from oracle import oracle
        lib = self.lib
        Q, C = self.queries() if QC is None else QC
        p, n = self.unmasked()
        cp, cn = self.state["cents"]
        both = len(p) > 0 and len(n) > 0
        fresh = {kn: lib.Model(self.ctx, p, n, cp, cn, kn) for kn in self.kns if kn <= len(p) + len(n)}
        for m in fresh.values():
            m.set_bandwidths(*self.state["bw"])
        rows = {"host": Q}
        if C is not None:
            rows["counts"] = rows["batch"] = oracle.normalize_counts(C.astype(np.int64))
        got_all = {}
        for path in self.paths:
            with self.ctx.options(**path):
                for kn, fm in fresh.items():
                    model = self.models[kn]
                    for method in ALL:
                        if method == "svm" and self.state["svm"] is None:
                            continue
                        tag = (what, path, kn, method)
                        got = self.run(model, Q, C, method)
                        want = self.run(self.svm_fresh if method == "svm" else fm, Q, C, method)
                        got_all[(str(path), kn, method)] = got
                        for entry, g in got.items():
                            w = want[entry]
                            if method == "density" and not both:
                                assert isinstance(g, lib.PhkError) and g.code == lib.PHK_ERR_ARG, (tag, entry, g)
                                continue
                            assert not isinstance(g, Exception), (tag, entry, g)
                            if method in ("knn", "svm"):
                                assert np.array_equal(g, w), (tag, entry, np.flatnonzero(g != w)[:10])
                            elif method == "density":
                                assert density_ref.close(g, w, F64), (tag, entry)
                            else:
                                assert helpers.rel_err(g, w) <= 1e-12, (tag, entry, helpers.rel_err(g, w))
        # the float64 restatements of the current rows, every entry point (the fused one on the counts it made)
        rows["fused"] = oracle.normalize_counts(self.syn_counts.astype(np.int64))
        allq = np.vstack([rows[e] for e in ("host", "counts", "fused") if e in rows])
        orc = Oracle(allq, p, n, cp, cn, self.state["bw"])
        offs, o = {}, 0
        for e in ("host", "counts", "fused"):
            if e in rows:
                offs[e] = (o, o + len(rows[e]))
                o += len(rows[e])
        offs["batch"] = offs.get("counts")
        for (path, kn, method), got in got_all.items():
            if method == "svm":
                continue
            for entry, g in got.items():
                if isinstance(g, Exception):
                    continue
                a, b = offs[entry]
                tag = (what, path, kn, method, entry)
                if method == "knn":
                    assert np.array_equal(g, orc.knn(kn)[a:b]), (tag, np.flatnonzero(g != orc.knn(kn)[a:b])[:10])
                elif method == "kmeans":
                    assert helpers.rel_err(g, orc.kmeans[a:b]) < RTOL, tag
                elif method == "combo":
                    assert helpers.rel_err(g, orc.knn(kn)[a:b] + orc.kmeans[a:b]) < RTOL, tag
                else:
                    assert density_ref.close(g, orc.density[a:b], F64), tag
        for m in fresh.values():
            m.close()
        return got_all

    def profile_counts(self, kn, method="knn"):
        """The kernels one score_counts call of the resident model runs on the held-out count queries (default knobs)."""
        _, C = self.queries()
        d_c = self.device.DeviceArray.from_host(self.ctx, C)
        d_s = self.device.DeviceArray(self.ctx, len(C), np.float64)
        self.ctx.profile_reset()
        self.ctx.profile_enable(True)
        self.device.score_counts(self.ctx, self.models[kn], d_c, len(C), method, d_s)
        self.ctx.sync()
        self.ctx.profile_enable(False)
        return self.ctx.profile()


def _assert_same(a, b, methods=("knn", "kmeans", "combo", "density")):
    for key, got in a.items():
        if key[2] not in methods:
            continue
        for entry, g in got.items():
            assert np.array_equal(g, b[key][entry]), (key, entry)


@pytest.mark.parametrize("tag", ["k4", "k5", "k6"])
def test_fold_state_in_any_call_order_equals_a_fresh_model(tag):
    from phamers_amd import _lib
    ctx = _lib.get_context()
    s = FoldState(ctx, tag, seed={"k4": 11, "k5": 12, "k6": 13}[tag])
    try:
        maskA, maskB = s.random_mask(0.2), s.random_mask(0.25)
        s.held = maskA
        fixed = s.queries()                 # the untouched model's scores are the end state's, for the same queries
        base = s.check("untouched", fixed)

        # 1. the cross-validation driver's order: centroids, then mask; an svm fit under the mask
        s.set_centroids(s.fold_centroids(maskA))
        s.set_mask(maskA)
        s.fit_svm()
        s.check("centroids then mask")
        if s.D == 256:
            prof = s.profile_counts(3)
            assert "phk_knn_f16h_kernel" in prof, sorted(prof)
        # 4. a mask replaced by another without clearing; the svm fit stays that of mask A (a snapshot)
        s.set_mask(maskB)
        s.check("mask replaced")
        # 2. mask, then centroids that move the k = 4 records' bias exponent (a one-hot centroid row: its bias dwarfs the
        # others): every block's bias pieces are rewritten, the masked ones must stay masked.  Measured at k = 4 with a
        # print in phk_model_update_centroids_f16: step 1 keeps bias_e at 9, this step takes it to 4, step 3 back to 9
        s.set_centroids(s.fold_centroids(maskB, hot=True))
        s.check("mask then centroids moving the bias exponent")
        if s.D == 256:
            assert "phk_knn_f16h_kernel" in s.profile_counts(3)
        else:
            assert not _i8_sweeps(s.profile_counts(3))     # no int8 sweep while a mask is set
        # 3. ... and centroids that move it back (the strided means: no bias beyond the train rows' own, 4 -> 9)
        s.set_centroids(s.fold_centroids(maskB))
        s.check("mask then centroids moving it back")
        # 7. bandwidths while a mask is set; 8. a refit under mask B, then a new mask without a refit
        s.set_bandwidths(0.02, 0.03)
        s.fit_svm()
        s.check("bandwidths and svm refit under the mask")
        s.set_mask(maskA)
        s.check("new mask, svm fit of the old one")
        # 6. exactly kn = 5 train rows left (both classes), then exactly 3 (the kn = 5 model refuses it)
        keep5 = np.ones(s.M, bool)
        keep5[[0, 1, 2, len(s.pos), len(s.pos) + 1]] = False
        s.set_mask(keep5)
        s.check("five train rows")
        keep3 = np.ones(s.M, bool)
        keep3[[1, len(s.pos), len(s.pos) + 2]] = False
        with pytest.raises(_lib.PhkError):
            s.models[5].set_column_mask(keep3)
        for kn in (1, 3):
            s.models[kn].set_column_mask(keep3)
        kns = s.kns
        s.kns = tuple(kn for kn in kns if kn != 5)
        s.state["mask"], s.held = keep3, keep3
        s.check("three train rows")
        s.kns = kns
        # a whole class held out: knn / kmeans / combo as the fresh model, density refused, fit_svm refused and the
        # previous fit kept
        no_neg = maskA.copy()
        no_neg[len(s.pos):] = True
        s.set_mask(no_neg)
        s.fit_svm()
        s.check("negative class masked out")
        # 5. clearing the mask and restoring the original centroids and bandwidths: the untouched model's scores
        s.set_mask(None)
        s.set_centroids((s.cp0, s.cn0))
        s.set_bandwidths(0.005, 0.01)
        again = s.check("cleared and restored", fixed)
        _assert_same(again, base)
    finally:
        s.close()


def test_int8_sweep_after_masks_and_centroid_replacement():
    """k = 5 with device-made counts, where the int8 sweep serves the untouched model: it stands down while a mask is set,
    comes back when the mask is cleared while the centroids were never replaced, and stays off after any
    phk_model_set_centroids (its operand is not rebuilt) -- with the scores of a fresh model throughout."""
    from oracle import oracle
    from phamers_amd import _lib, device
    ctx = _lib.get_context()
    k, D, n_ref, n_q = 5, 1024, 600, 500

    def device_counts(seed, n, L):
        T = n * L
        d_packed = device.DeviceArray(ctx, device.packed_words(T), np.uint32)
        d_off = device.DeviceArray(ctx, n + 1, np.uint64)
        device.synth_packed(ctx, seed, 0, n, L, d_packed, d_off)
        d_counts = device.DeviceArray(ctx, (n, D), np.uint32)
        device.count(ctx, d_packed, None, T, d_off, n, k, d_counts)
        return d_counts

    ref = device_counts(71, n_ref, 30000).to_host().astype(np.float64)
    ref[: n_ref // 2] *= 1.0 + 0.3 * np.sin(np.arange(D) * 0.37)
    ref /= ref.sum(axis=1, keepdims=True)
    pos, neg = ref[: n_ref // 2], ref[n_ref // 2:]

    def cents(p, n, hot=False):
        cp = np.stack([p[i::8].mean(axis=0) for i in range(8)])
        cn = np.stack([n[i::8].mean(axis=0) for i in range(8)])
        if hot:
            cp[0] = 0.0
            cp[0, 0] = 1.0
        return cp, cn

    c0 = cents(pos, neg)
    model = _lib.Model(ctx, pos, neg, *c0, 3)
    rng = np.random.default_rng(21)
    d_q = device_counts(72, n_q, 10000)
    q = oracle.normalize_counts(d_q.to_host().astype(np.int64))
    d_scores = device.DeviceArray(ctx, n_q, np.float64)

    def run(m, method):
        ctx.profile_reset()
        ctx.profile_enable(True)
        device.score_counts(ctx, m, d_q, n_q, method, d_scores, None)
        out = d_scores.to_host()
        ctx.profile_enable(False)
        return out, ctx.profile()

    def check(mask, cp_cn):
        p, n = (pos, neg) if mask is None else (pos[~mask[:len(pos)]], neg[~mask[len(pos):]])
        fresh = _lib.Model(ctx, p, n, *cp_cn, 3)
        out = {}
        for method in ("knn", "kmeans", "combo"):
            got, prof = run(model, method)
            want, _ = run(fresh, method)
            if method == "knn":
                assert np.array_equal(got, want)
                assert np.array_equal(got, oracle.knn_score_points(q, p, n, 3))
            else:
                assert helpers.rel_err(got, want) <= 1e-12, method
            out[method] = (got, _i8_sweeps(prof))
        assert helpers.rel_err(out["kmeans"][0], oracle.centroid_score_points_fast(q, *cp_cn)) < RTOL
        fresh.close()
        return out

    base = check(None, c0)
    assert base["knn"][1] and base["combo"][1]
    mask = rng.random(n_ref) < 0.3
    model.set_column_mask(mask)
    out = check(mask, c0)
    assert not out["knn"][1] and not out["combo"][1]
    model.set_column_mask(None)
    out = check(None, c0)
    assert out["knn"][1] and out["combo"][1]
    for method in base:
        assert np.array_equal(out[method][0], base[method][0]), method
    # after any set_centroids the int8 operand is stale for good (cen_replaced): the f16 sweep, the same scores
    model.set_column_mask(mask)
    c1 = cents(pos[~mask[:len(pos)]], neg[~mask[len(pos):]], hot=True)
    model.set_centroids(*c1)
    out = check(mask, c1)
    assert not out["knn"][1]
    model.set_column_mask(None)
    model.set_centroids(*c0)
    out = check(None, c0)
    assert not out["knn"][1] and not out["combo"][1]
    for method in base:
        assert np.array_equal(out[method][0], base[method][0]), method
    model.close()


@pytest.mark.parametrize("tag", ["k4", "k5"])
def test_cross_validation_with_device_kmeans_equals_fresh_fold_models(tag):
    """cross_validator(kmeans='gpu') on the resident model: every fold's scores equal a model built from that fold's train
    rows alone, with that fold's own centroids (learning.kmeans_gpu on the train rows of each class, deterministic)."""
    from phamers_amd import _lib, cross_validate, learning
    if tag == "k4":
        pos, neg = _ref_matrices()
        N, k_clusters = 5, 86
    else:
        g = helpers.load_npz("scoring_highdim.npz")
        pos, neg = g["pos_k5"], g["neg_k5"]
        N, k_clusters = 5, 6
    ctx = _lib.get_context()
    for method in ("knn", "kmeans", "combo"):
        v = cross_validate.cross_validator()
        v.positive_data, v.negative_data = pos, neg
        v.N, v.method, v.seed, v.kmeans, v.k_clusters = N, method, 17, "gpu", k_clusters
        ps, ns = v.cross_validate()
        assert v.model_uploads == 1
        for fold in range(N):
            out_p, out_n = v.positive_assignment == fold, v.negative_assignment == fold
            P, Nm = pos[~out_p], neg[~out_n]
            cp = learning.kmeans_gpu(P, k_clusters)[1] if method != "knn" else None
            cn = learning.kmeans_gpu(Nm, k_clusters)[1] if method != "knn" else None
            fresh = _lib.Model(ctx, P, Nm, cp, cn, k_neighbors=3)
            want = fresh.score(np.vstack((pos[out_p], neg[out_n])), method)
            fresh.close()
            got = np.concatenate((ps[out_p], ns[out_n]))
            if method == "knn":
                assert np.array_equal(got, want), (tag, fold)
            else:
                assert helpers.rel_err(got, want) <= 1e-12, (tag, method, fold)
