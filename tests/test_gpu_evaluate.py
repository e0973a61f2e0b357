"""GPU: the radix argsort, the integer ROC curve, the truth table and the reports built on them (phamers_amd/csrc/evaluate.hip,
learning.predictor_performance & co., cross_validator's reports, cut_validator) against tests/golden/evaluation.npz
(scikit-learn's roc_curve / auc and the reference's own functions) and the NumPy restatement tests/evaluate_ref.py."""
import os

import numpy as np
import pytest

from tests import evaluate_ref, helpers
from tests.test_evaluate_host import auc_bound

pytestmark = pytest.mark.gpu

TILE, MAX_BLOCKS = 4096, 512   # PHK_SORT_TILE, PHK_SORT_MAX_BLOCKS


@pytest.fixture(scope="module")
def golden():
    return helpers.load_npz("evaluation.npz")


@pytest.fixture(scope="module")
def beyond_one_grid():
    """More keys than one pass of the sort's largest grid covers: some workgroups take two tiles."""
    rng = np.random.RandomState(5)
    n = TILE * MAX_BLOCKS + 3
    return rng.normal(0.4, 1, n // 2), np.round(rng.normal(0, 1, n - n // 2), 4)


def test_library_constants():
    from phamers_amd import _lib
    assert (_lib.SORT_TILE, _lib.SORT_MAX_BLOCKS) == (TILE, MAX_BLOCKS) and evaluate_ref.TILE == TILE


@pytest.mark.parametrize("name", sorted(evaluate_ref.cases()))
def test_curves_equal_scikit_learn(golden, name):
    from phamers_amd import learning
    pos, neg = evaluate_ref.cases()[name]
    scores, labels = evaluate_ref.stack(pos, neg)
    for drop, sfx in ((True, ""), (False, "_all")):
        fps, tps, thr, area2 = learning.roc_points(scores, labels, drop)
        fpr, tpr, auc = learning.rates_from_points(fps, tps, area2)
        assert np.array_equal(fpr, golden[name + "_fpr" + sfx])
        assert np.array_equal(tpr, golden[name + "_tpr" + sfx])
        assert np.array_equal(thr, golden[name + "_thr" + sfx])
        assert area2 == evaluate_ref.roc_points(scores, labels, drop)[3]
        gap = abs(auc - float(golden[name + "_auc"]))
        print(name, drop, len(fpr), gap / 2.0 ** -53)
        assert gap <= auc_bound(len(fpr))
    fpr, tpr, auc = learning.predictor_performance(pos, neg)
    assert np.array_equal(fpr, golden[name + "_fpr"]) and np.array_equal(tpr, golden[name + "_tpr"])
    again = learning.predictor_performance(pos, neg)
    assert np.array_equal(again[0], fpr) and np.array_equal(again[1], tpr) and again[2] == auc   # bit-identical twice


def test_curve_beyond_one_grid_pass(beyond_one_grid):
    from sklearn.metrics import auc as sk_auc
    from phamers_amd import learning
    pos, neg = beyond_one_grid
    scores, labels = evaluate_ref.stack(pos, neg)
    fps, tps, thr, area2 = learning.roc_points(scores, labels, True)
    want = evaluate_ref.roc_points(scores, labels, True)
    assert np.array_equal(fps, want[0]) and np.array_equal(tps, want[1]) and np.array_equal(thr, want[2]) and area2 == want[3]
    fpr, tpr, auc = learning.rates_from_points(fps, tps, area2)
    assert abs(auc - sk_auc(fpr, tpr)) <= auc_bound(len(fpr))


def _argsort_both_ways(x):
    from phamers_amd import learning
    assert np.array_equal(learning.argsort_scores(x), np.argsort(x + 0.0, kind='stable'))
    assert np.array_equal(learning.argsort_scores(x, descending=True), np.argsort(-(x + 0.0), kind='stable'))


@pytest.mark.parametrize("name", sorted(evaluate_ref.cases()))
def test_argsort_on_the_curve_inputs(name):
    _argsort_both_ways(evaluate_ref.stack(*evaluate_ref.cases()[name])[0])


def test_argsort_shapes_ties_and_single_bytes(beyond_one_grid):
    from phamers_amd import learning
    rng = np.random.RandomState(9)
    assert learning.argsort_scores(np.zeros(0)).shape == (0,)
    _argsort_both_ways(np.array([3.5]))
    _argsort_both_ways(np.concatenate(beyond_one_grid))
    ties = rng.choice([-1.0, 1.0], 3 * 2 ** 16 + 5)                 # more than 2^16 equal keys of each value
    ties[::1000] = 0.5
    _argsort_both_ways(ties)
    _argsort_both_ways(np.full(2 ** 16 + 9, -0.0))
    base = np.float64(1.5).view(np.uint64)
    low = (base + rng.randint(0, 256, 3 * TILE + 5).astype(np.uint64)).view(np.float64)      # images differ in the bottom byte only
    assert len(np.unique(low)) > 200
    _argsort_both_ways(low)
    top = np.array([0x0000000000000000, 0x0100000000000000, 0x3f00000000000000, 0x7e00000000000000, 0x8100000000000000,
                    0xbf00000000000000, 0xfe00000000000000], dtype=np.uint64).view(np.float64)    # ... in the top byte only
    _argsort_both_ways(top[rng.randint(0, len(top), 2 * TILE + 3)])


def test_non_finite_scores_raise_and_an_empty_class_gives_nan():
    from phamers_amd import learning
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError):
            learning.predictor_performance([0.5, bad], [0.1, 0.2, 0.3])
        with pytest.raises(ValueError):
            learning.argsort_scores([0.5, 0.25, bad])
    fpr, tpr, auc = learning.predictor_performance([0.5, 0.7], [])
    assert np.isnan(fpr).all() and np.array_equal(tpr, [0.0, 0.5, 1.0]) and np.isnan(auc)
    fpr, tpr, auc = learning.predictor_performance([], [0.5, 0.7])
    assert np.isnan(tpr).all() and np.array_equal(fpr, [0.0, 0.5, 1.0]) and np.isnan(auc)


@pytest.mark.parametrize("name", ["normal", "pm1", "rounded", "equal", "one_many", "cv_n7_knn", "cv_n20_combo"])
def test_truth_table_and_metrics_equal_the_reference(golden, name):
    from phamers_amd import learning
    if name.startswith("cv_"):
        cv = helpers.load_npz("cross_validation.npz")
        pos, neg = cv["pos_scores_" + name[3:]], cv["neg_scores_" + name[3:]]
    else:
        pos, neg = evaluate_ref.cases()[name]
    for i, th in enumerate(golden[name + "_thresholds"]):
        assert list(learning.get_truth_table(pos, neg, threshold=th)) == list(golden[name + "_truth"][i])
        want = golden[name + "_metrics"][i]
        tp, fp, fn, tn = want[:4]
        if tp + fp == 0 or tn + fn == 0:        # the reference's zero denominators
            with pytest.raises(ZeroDivisionError):
                learning.get_predictor_metrics(pos, neg, threshold=th)
            continue
        m = learning.get_predictor_metrics(pos, neg, threshold=th)
        assert tuple(m.keys()) == evaluate_ref.METRIC_NAMES == learning.METRIC_NAMES
        assert [m[k] for k in m] == list(want) and m.tpr == m['tpr'] == want[4]


def test_cross_validator_reports(golden, tmp_path):
    from phamers_amd import cross_validate, kmer, learning
    z = helpers.load_npz("cross_validation.npz")
    f = helpers.load_npz("ref_features.npz")
    pos = kmer.normalize_counts(f["pos_counts"].astype(np.int64))
    neg = kmer.normalize_counts(f["neg_counts"].astype(np.int64))
    tag = "n7_knn"
    seed, N, n_pos, n_neg = (int(x) for x in z["meta_" + tag])
    v = cross_validate.cross_validator()
    v.positive_data, v.negative_data = pos.copy(), neg.copy()
    v.positive_ids, v.negative_ids = ['p%04d' % i for i in range(len(pos))], ['n%04d' % i for i in range(len(neg))]
    v.equalize_reference, v.N, v.method, v.seed = True, N, "knn", seed
    v.output_directory = str(tmp_path / "out")
    v.cross_validate()
    fpr, tpr, auc = v.performance()
    assert np.array_equal(fpr, golden["cv_%s_fpr" % tag]) and np.array_equal(tpr, golden["cv_%s_tpr" % tag])
    assert abs(auc - float(golden["cv_%s_auc" % tag])) <= auc_bound(len(fpr))
    v.make_metrics_file()
    v.make_summary_file()
    assert open(v.get_metric_filename()).read() == str(golden["cv_%s_metrics_text" % tag])
    assert open(v.get_summary_filename()).read() == str(golden["cv_%s_summary" % tag])
    labels = {i: "label-" + i for i in v.positive_ids}
    v.make_summary_file(id_label_map=labels)
    lines = open(v.get_summary_filename()).read().split("\n")
    want = str(golden["cv_%s_summary" % tag]).split("\n")
    assert lines[0] == want[0] and lines[1:] == [w + "\tlabel-" + w.split("\t")[0] for w in want[1:]]
    # all algorithms: the same fold plan per method as separate seeded runs
    v.positive_data, v.negative_data = pos[:600].copy(), neg[:600].copy()
    v.positive_ids, v.negative_ids = v.positive_ids[:600], v.negative_ids[:600]
    v.N, v.seed, v.kmeans, v.k_clusters, v.methods = 3, 11, 'gpu', 12, ['knn', 'kmeans']
    results = v.cross_validate_all_algorithms()
    assert list(results) == ['knn', 'kmeans']
    for method in v.methods:
        w = cross_validate.cross_validator()
        w.positive_data, w.negative_data = pos[:600].copy(), neg[:600].copy()
        w.N, w.seed, w.kmeans, w.k_clusters, w.method = 3, 11, 'gpu', 12, method
        alone = learning.predictor_performance(*w.cross_validate())
        assert results[method][2] == alone[2] and np.array_equal(results[method][0], alone[0])
        assert 0.5 < results[method][2] <= 1.0


def _synthetic_records(rng, cut, weights, count):
    lengths = [0, cut - 1, cut, cut + 1, 3 * cut + 7] * (count // 5)
    seqs = []
    for L in lengths:
        s = rng.choice(list("ATGC"), L, p=weights)
        if L > cut + 1:
            s[cut - 3:cut + 4] = "N"            # a run of N across a piece boundary
        seqs.append("".join(s))
    return seqs


@pytest.mark.parametrize("cut,k", [(64, 4), (1000, 4), (64, 5)])
def test_count_cuts_equals_counting_the_pieces(cut, k):
    from phamers_amd import kmer
    rng = np.random.RandomState(cut + k)
    seqs = _synthetic_records(rng, cut, [0.25] * 4, 40)
    ids, counts = kmer.count_cuts(seqs, k, cut)
    pieces, want_ids = [], []
    for r, s in enumerate(seqs):
        for i in range(len(s) // cut):
            pieces.append(s[i * cut:(i + 1) * cut])
            want_ids.append("%d_%d" % (r, i))
    assert ids == want_ids and counts.shape == (len(pieces), 4 ** k)
    assert np.array_equal(counts, kmer.count(pieces, k))
    assert kmer.count_cuts(["ACGT" * 3], k, cut)[1].shape == (0, 4 ** k)


def test_cut_files_and_cut_response(tmp_path):
    from phamers_amd import cross_validate, cut_validator, fileIO, kmer, learning
    rng = np.random.RandomState(2)
    fastas = {}
    for kind, weights in (("phage", [0.35, 0.35, 0.15, 0.15]), ("bacteria", [0.15, 0.15, 0.35, 0.35])):
        path = str(tmp_path / (kind + ".fasta"))
        with open(path, "w") as f:
            for r in range(12):
                f.write(">%s_%d\n%s\n" % (kind, r, "".join(rng.choice(list("ATGC"), 900 + 37 * r, p=weights))))
        fastas[kind] = path
    t = cut_validator.tester()
    t.cut_directory, t.N_fold = str(tmp_path / "cuts"), 3
    t.validator = cross_validate.cross_validator()
    t.validator.method, t.validator.seed = 'knn', 4
    written = t.make_cut_files(fastas["phage"], fastas["bacteria"], [200, 400])
    ids, _ = kmer.count_cuts(fastas["phage"], 4, 400)
    assert ids[:3] == ["phage_0_0", "phage_0_1", "phage_1_0"]
    assert sorted(os.path.basename(w) for w in written) == [
        "bacteria_kmer_count_k4_c200_s0.csv", "bacteria_kmer_count_k4_c400_s0.csv", "phage_kmer_count_k4_c200_s0.csv",
        "phage_kmer_count_k4_c400_s0.csv"]
    ids, rows = fileIO.read_feature_file(written[0], old=True)
    assert set(ids) == {"No_ID"} and rows.shape[1] == 256 and (rows.sum(axis=1) == 200 - 3).all()
    aucs = t.test_cut_response()
    assert sorted(aucs) == [200, 400]
    for cut in (200, 400):
        w = cross_validate.cross_validator()
        w.method, w.seed, w.N = 'knn', 4, 3
        w.positive_data = fileIO.read_feature_file(os.path.join(t.cut_directory, "phage_kmer_count_k4_c%d_s0.csv" % cut), normalize=True, old=True)[1]
        w.negative_data = fileIO.read_feature_file(os.path.join(t.cut_directory, "bacteria_kmer_count_k4_c%d_s0.csv" % cut), normalize=True, old=True)[1]
        assert aucs[cut] == learning.predictor_performance(*w.cross_validate())[2]
        assert aucs[cut] > 0.9
