"""CPU-only: the NumPy restatement of the integer ROC method (tests/evaluate_ref.py) against the scikit-learn fixture
tests/golden/evaluation.npz, and the host bookkeeping of the cut validator."""
import numpy as np
import pytest

from tests import evaluate_ref, helpers


@pytest.fixture(scope="module")
def golden():
    return helpers.load_npz("evaluation.npz")


def auc_bound(m):
    """|auc - scikit-learn's| <= 4 m 2^-53: at most three roundings per trapezoid term, on values <= 1, over m terms."""
    return 4 * m * 2.0 ** -53


def test_restatement_is_bit_equal_to_the_golden_curves(golden):
    for name, (pos, neg) in evaluate_ref.cases().items():
        scores, labels = evaluate_ref.stack(pos, neg)
        for drop, sfx in ((True, ""), (False, "_all")):
            fps, tps, thr, area2 = evaluate_ref.roc_points(scores, labels, drop)
            fpr, tpr, auc = evaluate_ref.rates(fps, tps, area2)
            assert np.array_equal(fpr, golden[name + "_fpr" + sfx]), name
            assert np.array_equal(tpr, golden[name + "_tpr" + sfx]), name
            assert np.array_equal(thr, golden[name + "_thr" + sfx]), name
            gap = abs(auc - float(golden[name + "_auc"]))
            print(name, drop, len(fpr), gap / 2.0 ** -53)
            assert gap <= auc_bound(len(fpr)), (name, gap)


def test_restatement_truth_tables_equal_the_reference(golden):
    for name, (pos, neg) in evaluate_ref.cases().items():
        for i, th in enumerate(golden[name + "_thresholds"]):
            counts = evaluate_ref.truth_counts(pos, neg, th)
            assert list(evaluate_ref.truth_table(*counts)) == list(golden[name + "_truth"][i]), (name, th)
            assert list(map(float, counts)) == list(golden[name + "_metrics"][i][:4])


def test_cutsize_from_the_reference_example_name():
    from phamers_amd import cut_validator
    assert cut_validator.get_cutsize_from_filename("phage_kmer_count_k4_c100000_s0.csv") == 100000
    assert cut_validator.get_cutsize_from_filename("/some/dir/bacteria_kmer_count_k4_c64_s0.csv") == 64
    with pytest.raises(ValueError):
        cut_validator.get_cutsize_from_filename("phage_kmer_count.csv")


def test_cut_plan_rows_tails_and_ids():
    from phamers_amd import kmer
    cut = 64
    lengths = [0, cut - 1, cut, cut + 1, 3 * cut + 7, 10, 2 * cut]
    offsets, keep, owner, index = kmer.cut_plan(lengths, cut)
    pieces, want_keep, want_owner, want_index, at = [], [], [], [], 0
    for r, L in enumerate(lengths):
        for i, s in enumerate(range(0, L, cut)):
            if min(cut, L - s) == cut:
                want_keep.append(len(pieces))
                want_owner.append(r)
                want_index.append(i)
            pieces.append(at + s)
        at += L
    assert list(offsets) == pieces + [at]
    assert list(keep) == want_keep and list(owner) == want_owner and list(index) == want_index
    assert ["%d_%d" % p for p in zip(owner, index)] == ["2_0", "3_0", "4_0", "4_1", "4_2", "6_0", "6_1"]
    assert all(int(offsets[k + 1] - offsets[k]) == cut for k in keep)
    offsets, keep, _, _ = kmer.cut_plan([5, 0], 64)
    assert list(offsets) == [0, 5] and len(keep) == 0
    with pytest.raises(ValueError):
        kmer.cut_plan([5], 0)
