"""Batched per-contig placement (phk_placement_run, learning.place_contigs) and the taxonomy prediction built on it, on
the GPU: parity with the reference's per-contig results (tests/golden/placement.npz / .json), equality with the existing
single-problem device paths, invariance under batching, the declined problems, odd shapes."""
import re

import numpy as np
import pytest

from oracle import oracle
from tests import helpers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    ref = helpers.load_npz("ref_features.npz")
    pos = oracle.normalize_counts(ref["pos_counts"].astype(np.int64))
    neg = oracle.normalize_counts(ref["neg_counts"].astype(np.int64))
    g = helpers.load_npz("placement.npz")
    contigs = np.vstack((neg[g["neg_rows"]], g["uniform_rows"], pos[g["dup_rows"]]))
    return pos, contigs, g


@pytest.fixture(scope="module")
def placed(probe):
    from phamers_amd import learning
    pos, contigs, g = probe
    details = {}
    recs = learning.place_contigs(pos, contigs, int(g["k_clusters"][0]), _details=details)
    return recs, details


def _golden_sils(g, prefix=""):
    lens = g[prefix + "sil_len"]
    cuts = np.concatenate(([0], np.cumsum(lens)))
    return [g[prefix + "sil"][cuts[i]:cuts[i + 1]] for i in range(len(lens))]


def _check_records(recs, assignments, sils):
    for b, rec in enumerate(recs):
        a = assignments[b].astype(np.int64)
        assert np.array_equal(rec["labels"], a), (b, rec["route"])
        assert rec["cluster"] == a[-1]
        assert np.array_equal(rec["members"], np.flatnonzero(a[:-1] == a[-1]))
        assert rec["silhouettes"].shape == sils[b].shape
        err = np.max(np.abs(rec["silhouettes"] - sils[b]))
        print("contig %d route %s silhouette err %.3g" % (b, rec["route"], err))
        assert err <= 1e-8


def test_parity_with_the_reference_on_the_probe_set(probe, placed):
    pos, contigs, g = probe
    recs, _ = placed
    _check_records(recs, g["assignments"], _golden_sils(g))


def test_at_most_two_probe_contigs_take_the_host_route(placed):
    recs, details = placed
    routes = [r["route"] for r in recs]
    print("routes:", routes)
    print("seed margins:", details["seed_margin"], "gaps:", details["min_gap"], "status:", details["status"],
          "sweeps:", details["n_iter"])
    assert routes.count("host") <= 2
    assert len(set(details["n_iter"].tolist())) > 1        # problems of one batch converge in different sweep counts


def test_duplicates_of_reference_rows_go_to_the_host(placed):
    from phamers_amd import _lib
    recs, details = placed
    for b in (18, 19):
        assert recs[b]["route"] == "host" and details["status"][b] & _lib.PLACEMENT_DUPLICATE
    assert not (details["status"][:18] & _lib.PLACEMENT_DUPLICATE).any()


@pytest.mark.parametrize("name", ["s24", "s130"])
def test_parity_with_the_reference_on_the_synthetic_sets(name):
    from phamers_amd import learning
    g = helpers.load_npz("placement.npz")
    recs = learning.place_contigs(g[name + "_X"], g[name + "_Z"], int(g[name + "_k"][0]))
    print(name, [r["route"] for r in recs])
    _check_records(recs, g[name + "_assignments"], _golden_sils(g, name + "_"))


def test_taxonomy_predictor_reproduces_the_golden_dictionary(probe):
    from phamers_amd import analysis
    pos, contigs, g = probe
    doc = helpers.load_json("placement.json")
    an = analysis.taxonomy_predictor(pos, doc["lineages"], contigs, np.array(doc["ids"]))
    assert an.k_clusters == 86 and an.phylogeny_names[4] == "Sub-Family"
    got = an.get_taxonomy_prediction_dict()
    want = {k: v for k, v in doc["predictions"].items() if v is not None}
    assert got is an.taxonomy_prediction_dict and set(got) == set(want) and len(want) >= 3
    assert set(an.cluster_silhouette_map) == set(an.cluster_lineage_map) == set(doc["ids"])
    number = re.compile(r"[-+]?\d+\.?\d*(?:[eE][-+]?\d+)?")
    for id, w in want.items():
        (kind, res, ratio), text = got[id]
        assert kind == w["kind"] and ratio == w["ratio"] and res[2] == w["dof"]
        assert abs(res[0] - w["chi2"]) <= 1e-12 * abs(w["chi2"]) and abs(res[1] - w["p"]) <= 1e-12 * abs(w["p"])
        assert np.allclose(res[3], w["expected"], rtol=1e-14, atol=0)
        assert number.sub("#", text) == number.sub("#", w["text"])
        a, b = [float(x) for x in number.findall(text)], [float(x) for x in number.findall(w["text"])]
        assert len(a) == len(b)
        for x, y in zip(a[:-1], b[:-1]):                 # percentage, digits of the names, the three silhouette figures
            assert abs(x - y) <= 1e-8, (text, w["text"])
        assert abs(a[-1] - b[-1]) <= 1e-12 * abs(b[-1]), (text, w["text"])      # p
    # ids_to_diagram narrows the prediction
    an.ids_to_diagram = [doc["ids"][3]]
    assert set(an.get_taxonomy_prediction_dict()) == {doc["ids"][3]} & set(want)
    assert set(an.cluster_silhouette_map) == {doc["ids"][3]}


def test_equality_with_the_single_problem_paths(probe, placed):
    """Device-route problems: seeds = kmeans_plusplus_seeds', labels / sweeps / min_gap = phk_kmeans_lloyd's for the same
    centred rows and seeds, silhouettes within 1e-11 of learning.cluster_silhouettes (another summation order)."""
    import ctypes
    from phamers_amd import _lib, learning
    pos, contigs, g = probe
    recs, details = placed
    k = int(g["k_clusters"][0])
    ctx = _lib.get_context()
    checked = 0
    for b in range(0, len(recs)):
        if recs[b]["route"] != "device":
            continue
        X = np.vstack((pos, contigs[b][None, :]))
        Xc = X - X.mean(axis=0)
        init, idx = learning.kmeans_plusplus_seeds(Xc, k, np.random.RandomState(learning.kmeans_seed))
        assert np.array_equal(details["seeds"][b], idx), b
        tol_abs = float(np.mean(np.var(Xc, axis=0)) * 1e-4)
        labels = np.empty(X.shape[0], dtype=np.uint32)
        n_iter, n_empty, min_gap = ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
        _lib.check(ctx.lib.phk_kmeans_lloyd(ctx.handle, _lib.ptr(np.ascontiguousarray(Xc)), X.shape[0], X.shape[1], k,
                                            _lib.ptr(np.ascontiguousarray(init)), tol_abs, 300, None, _lib.ptr(labels),
                                            ctypes.byref(n_iter), ctypes.byref(n_empty), ctypes.byref(min_gap)))
        assert np.array_equal(details["labels"][b], labels), b
        assert details["n_iter"][b] == n_iter.value and details["min_gap"][b] == min_gap.value and n_empty.value == 0, b
        sil = learning.cluster_silhouettes(X, labels.astype(np.int32), int(labels[-1]))
        err = np.max(np.abs(sil - recs[b]["silhouettes"]))
        print("contig %d sweeps %d gap %.3g silhouettes vs single-problem path %.3g" % (b, n_iter.value, min_gap.value, err))
        assert err <= 1e-11
        checked += 1
    assert checked >= 18


def _same(a, b):
    return (np.array_equal(a["labels"], b["labels"]) and np.array_equal(a["silhouettes"], b["silhouettes"])
            and a["route"] == b["route"] and a["cluster"] == b["cluster"])


def test_batch_invariance_and_rerun(probe, placed):
    from phamers_amd import _lib, learning
    pos, contigs, g = probe
    recs, details = placed
    k = int(g["k_clusters"][0])
    ctx = _lib.get_context()
    sub = [1, 5, 12, 14, 3]
    first, draws = learning.placement_draws(pos.shape[0] + 1, k)
    pl = _lib.Placement(ctx, pos)
    try:
        whole = pl.run(contigs[sub], k, first, draws)
        again = pl.run(contigs[sub], k, first, draws)
        rev = pl.run(contigs[sub[::-1]], k, first, draws)
        ctx.profile_enable(True)
        ctx.profile_reset()
        try:
            split = pl.run(contigs[sub], k, first, draws, chunk=2)       # chunks of 2, 2, 1 problems
            launches = {name: v[1] for name, v in ctx.profile().items()}
        finally:
            ctx.profile_enable(False)
        ones = [pl.run(contigs[[i]], k, first, draws) for i in sub]
    finally:
        pl.close()
        pl.close()                                                       # twice is harmless
    assert launches["pl_dup_kernel"] == 3 and launches["pl_seed_dist_kernel"] == 3 * k
    assert len(set(whole["n_iter"].tolist())) > 1
    for key in whole:
        m = whole["n_members"]
        def cut(o, j):
            return o[key][j][:m[j]] if key == "sil" else o[key][j]
        for j in range(len(sub)):
            assert np.array_equal(cut(whole, j), details[key][sub[j]][:m[j]] if key == "sil" else details[key][sub[j]]), key
            assert np.array_equal(cut(whole, j), cut(again, j)), key
            assert np.array_equal(cut(whole, j), cut(split, j)), key
            assert np.array_equal(cut(whole, j), rev[key][len(sub) - 1 - j][:m[j]] if key == "sil" else rev[key][len(sub) - 1 - j]), key
            assert np.array_equal(cut(whole, j), ones[j][key][0][:m[j]] if key == "sil" else ones[j][key][0]), key
    with pytest.raises(ValueError):
        pl.run(contigs[:1], k, first, draws)                             # closed


def _host_answer(X, z, k):
    from phamers_amd import learning
    app = np.vstack((X, z[None, :]))
    a = np.asarray(learning.kmeans(app, k))
    return a, learning.cluster_silhouettes(app, a, a[-1])


def test_exact_tie_goes_to_the_host():
    """Four rows at -1, four at +1, the contig at 0: the seeds are one row of each side (drawn from rows with equal
    potentials), and the contig is equidistant from the two centres."""
    from phamers_amd import learning
    X = np.array([[-1.0, 0.0]] * 4 + [[1.0, 0.0]] * 4)
    z = np.array([0.0, 0.0])
    details = {}
    rec = learning.place_contigs(X, z[None, :], 2, _details=details)[0]
    print("tie set: margin", details["seed_margin"], "gap", details["min_gap"], "status", details["status"])
    assert rec["route"] == "host"
    assert details["seed_margin"][0] < learning.SEED_MIN_MARGIN or details["min_gap"][0] < learning.KMEANS_MIN_GAP
    a, sil = _host_answer(X, z, 2)
    assert np.array_equal(rec["labels"], a) and np.array_equal(rec["silhouettes"], sil)


def test_empty_cluster_goes_to_the_host():
    """Three distinct locations, four clusters: the fourth centre repeats an earlier one and its cluster stays empty."""
    import warnings
    from phamers_amd import _lib, learning
    X = np.array([[0.0, 0, 0]] * 5 + [[4.0, 0, 1]] * 5 + [[0, 5.0, 2]] * 5)
    z = np.array([4.0, 0.0, 1.0])
    details = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")       # (scikit-learn: fewer distinct points than clusters)
        rec = learning.place_contigs(X, z[None, :], 4, _details=details)[0]
        a, sil = _host_answer(X, z, 4)
    print("empty set: status", details["status"], "margin", details["seed_margin"])
    assert rec["route"] == "host" and details["status"][0] & _lib.PLACEMENT_EMPTY
    assert np.array_equal(rec["labels"], a) and np.array_equal(rec["silhouettes"], sil)


@pytest.mark.parametrize("n,D,k,B", [(99, 70, 2, 1), (140, 33, 5, 3), (300, 130, 7, 2), (40, 5, 3, 4)])
def test_odd_shapes_against_the_single_problem_paths(n, D, k, B):
    from phamers_amd import learning
    rng = np.random.RandomState(n + D)
    centres = rng.uniform(-1, 1, (k + 1, D))
    X = centres[rng.randint(0, k + 1, n)] + 0.3 * rng.randn(n, D)
    Z = centres[rng.randint(0, k + 1, B)] + 0.3 * rng.randn(B, D)
    recs = learning.place_contigs(X, Z, k)
    print([r["route"] for r in recs])
    assert len(recs) == B
    for b in range(B):
        a, sil = _host_answer(X, Z[b], k)
        assert np.array_equal(recs[b]["labels"], a)
        assert np.max(np.abs(recs[b]["silhouettes"] - sil)) <= 1e-11
    assert sum(r["route"] == "device" for r in recs) >= 1


def test_errors_and_empty_batch():
    from phamers_amd import learning
    X = np.random.RandomState(0).rand(30, 9)
    assert learning.place_contigs(X, np.empty((0, 9)), 3) == []
    with pytest.raises(ValueError, match="n_clusters=32"):
        learning.place_contigs(X, np.zeros((1, 9)), 32)
    bad = np.zeros((2, 9))
    bad[1, 4] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        learning.place_contigs(X, bad, 3)


def test_sklearn_mode_takes_the_host_route(monkeypatch):
    from phamers_amd import learning
    g = helpers.load_npz("placement.npz")
    monkeypatch.setenv("PHAMERS_KMEANS", "sklearn")
    recs = learning.place_contigs(g["s24_X"], g["s24_Z"][:2], int(g["s24_k"][0]))
    assert [r["route"] for r in recs] == ["host", "host"]
    _check_records(recs, g["s24_assignments"][:2], _golden_sils(g, "s24_")[:2])


def test_a_placement_beside_a_live_model_leaves_its_scores_alone(probe):
    from phamers_amd import _lib, learning
    pos, contigs, g = probe
    ref = helpers.load_npz("ref_features.npz")
    neg = oracle.normalize_counts(ref["neg_counts"].astype(np.int64))
    ctx = _lib.get_context()
    model = _lib.Model(ctx, pos, neg, k_neighbors=3)
    try:
        q = contigs[:16]
        before = model.score(q, "knn")
        pl = _lib.Placement(ctx, pos)
        try:
            first, draws = learning.placement_draws(pos.shape[0] + 1, 86)
            pl.run(contigs[:3], 86, first, draws)
            during = model.score(q, "knn")
        finally:
            pl.close()
        after = model.score(q, "knn")
    finally:
        model.close()
    want = oracle.score_points(q, pos, neg, "knn", 3, None, None)
    assert np.array_equal(before, during) and np.array_equal(before, after)
    assert np.array_equal(before, want)      # knn scores are votes: -1.0 / +1.0
