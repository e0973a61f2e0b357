"""Strand fold, host side: the column permutation, the identity fold(count(s)) == count(s) + count(revcomp(s)) on the CPU
oracle for every kind of string, and the argument errors of the Python layer that need no device."""
import numpy as np
import pytest

from tests import strands_ref

KS = [1, 2, 3, 4, 5, 6, 7]


@pytest.mark.parametrize("k", KS)
def test_rc_is_an_involution_with_the_palindromes_as_fixed_points(k):
    from phamers_amd import transform_kmers
    rc = strands_ref.rc_table(k)
    assert np.array_equal(np.sort(rc), np.arange(4 ** k))
    assert np.array_equal(rc[rc], np.arange(4 ** k))
    assert int((rc == np.arange(4 ** k)).sum()) == (4 ** (k // 2) if k % 2 == 0 else 0)
    assert np.array_equal(rc, transform_kmers.exact_indices(k, True, True))


def test_rc_of_named_kmers():
    from oracle import oracle
    mers = oracle.kmers(3)
    rc = strands_ref.rc_table(3)
    for c, m in enumerate(mers):
        assert mers[rc[c]] == strands_ref.revcomp(m)
    assert strands_ref.revcomp("AAGCNtx") == "xtNGCTT"


@pytest.mark.parametrize("k", KS)
def test_fold_of_a_count_is_the_count_of_both_strands(k):
    """Lengths 0, k-1, k, k+1, 37, 500 over 'ATGCNatn': N and lower case are dropped by the reference's rule on both
    strands alike (a window holds an invalid character exactly when its mirror image does)."""
    from oracle import oracle
    rng = np.random.RandomState(k)
    for L in (0, k - 1, k, k + 1, 37, 500):
        s = "".join(rng.choice(list("ATGCNatn"), L, p=[0.23, 0.23, 0.23, 0.23, 0.02, 0.02, 0.02, 0.02])) if L else ""
        fwd = np.asarray(oracle.count_string(s, k), dtype=np.int64)
        rev = np.asarray(oracle.count_string(strands_ref.revcomp(s), k), dtype=np.int64)
        folded = strands_ref.fold(fwd)
        assert np.array_equal(folded, fwd + rev), (k, L)
        assert folded.sum() == 2 * fwd.sum()
        assert np.array_equal(strands_ref.fold(rev), folded)       # the two strands fold to the same row


def test_iupac_and_other_characters_stay_invalid_on_both_strands():
    from oracle import oracle
    s = "ATGRYCCGTANNKMSWacgtTTGACCA-GGT*AC"
    for k in (2, 4):
        fwd = np.asarray(oracle.count_string(s, k), dtype=np.int64)
        rev = np.asarray(oracle.count_string(strands_ref.revcomp(s), k), dtype=np.int64)
        assert fwd.sum() > 0 and np.array_equal(strands_ref.fold(fwd), fwd + rev)


def test_argument_errors_that_need_no_device():
    from phamers_amd import kmer, transform_kmers
    with pytest.raises(TypeError):
        transform_kmers.fold_strands(np.ones((2, 16)))                     # float rows
    with pytest.raises(TypeError):
        transform_kmers.fold_strands(np.ones((2, 16), dtype=np.float32))
    with pytest.raises(ValueError):
        transform_kmers.fold_strands(np.ones((2, 100), dtype=np.int64))    # not 4^k
    with pytest.raises(ValueError):
        transform_kmers.fold_strands(np.ones((2, 4 ** 8), dtype=np.int8))  # k above the kernels' limit
    with pytest.raises(ValueError):
        transform_kmers.fold_strands(np.ones(16, dtype=np.int64))          # a matrix is expected
    for call in (lambda: kmer.count_string("ACGT", 2, symbols="ACGT", both_strands=True),
                 lambda: kmer.count(["ACGT", "AC"], 2, symbols="TAGC", both_strands=True),
                 lambda: kmer.count_file("nope.fasta", 2, symbols="ACGT", both_strands=True),
                 lambda: kmer.count_directory(".", 2, symbols="ACGT", both_strands=True),
                 lambda: kmer.count_cuts(["ACGT"], 2, 2, symbols="ACGT", both_strands=True),
                 lambda: kmer.count_windows(["ACGT"], 2, 2, 1, symbols="ACGT", both_strands=True)):
        with pytest.raises(NotImplementedError):
            call()


def test_command_lines_take_the_option():
    from phamers_amd import kmer, phamer, windows
    assert kmer._parser().parse_args(["in.fa", "out.csv", "--both_strands"]).both_strands
    assert not kmer._parser().parse_args(["in.fa", "out.csv"]).both_strands
    assert phamer._parser().parse_args(["-in", "x", "--both_strands", "--gpus", "2"]).both_strands
    assert not phamer._parser().parse_args(["-in", "x"]).both_strands
    assert windows._parser().parse_args(["-in", "g.fa", "-out", "o", "--both_strands"]).both_strands
    assert not windows._parser().parse_args(["-in", "g.fa", "-out", "o"]).both_strands
    assert phamer.phamer_scorer().both_strands is False
