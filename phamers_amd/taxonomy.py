"""
taxonomy.py -- the lineage statistics of PhaMers' scripts/taxonomy.py that the taxonomy prediction needs (host only):

    find_enriched_classification(test_lineages, base_lineages, depth)   scripts/taxonomy.py:208-245
    extend_lineages(lineages)                                           scripts/taxonomy.py:112-122
    deepest_classification(lineages)                                    scripts/taxonomy.py:248-254

The NCBI lookups and the charts of scripts/taxonomy.py are out of scope.
"""
import math

import numpy as np


def deepest_classification(lineages):
    """The number of ranks of the longest lineage."""
    return max([len(lineage) for lineage in lineages])


def extend_lineages(lineages):
    """Every lineage padded with its own last rank to the length of the longest one (in place, and returned)."""
    lineages = list(lineages) if not isinstance(lineages, list) else lineages
    max_classification = deepest_classification(lineages)
    for i in range(len(lineages)):
        lineage = lineages[i]
        lineages[i] = np.concatenate((lineage, list(np.repeat(lineage[-1], max_classification - len(lineage)))))
    return lineages


def chi2_contingency_2x2(x):
    """``scipy.stats.chi2_contingency(x)`` for a 2 x 2 table of counts: (chi2, p, dof, expected) with Yates' continuity
    correction (each |observed - expected| reduced by min(0.5, itself)) and one degree of freedom, whose survival function
    is ``erfc(sqrt(chi2 / 2))`` -- no SciPy on the product path.  ValueError for a zero expected frequency, as SciPy."""
    x = np.asarray(x, dtype=np.float64)
    total = x.sum()
    expected = np.outer(x.sum(axis=1), x.sum(axis=0)) / total
    if (expected == 0).any():
        raise ValueError("The internally computed table of expected frequencies has a zero element.")
    diff = expected - x
    observed = x + np.sign(diff) * np.minimum(0.5, np.abs(diff))
    chi2 = float(((observed - expected) ** 2 / expected).sum())
    p = math.erfc(math.sqrt(chi2 / 2.0))
    return chi2, p, 1, expected


def find_enriched_classification(test_lineages, base_lineages, depth):
    """Is some taxon at rank ``depth`` enriched in ``test_lineages`` (a cluster's) against ``base_lineages`` (all)?
    (scripts/taxonomy.py:208-245.)  A taxon counts when it holds at least half of the test set, a larger share than in the
    base set, and the 2 x 2 table [[test others, test taxon], [base others, base taxon]] differs from independence with
    p <= 0.05 (chi-squared with Yates' correction); a taxon that is the whole base set has p = 1.  Returns
    ``(kind, (chi2, p, dof, expected), ratio)`` or ``(None, None, None)``.

    The reference walks ``set(all_kinds)`` in hash order and returns the first taxon that passes; this walks the taxa
    sorted.  The outcome can differ only when two taxa each hold exactly half of the test set and both pass."""
    no_enrichment_return = (None, None, None)
    test_kinds = [test_lineages[i][depth] for i in range(len(test_lineages))]
    if len(test_lineages) == 0:
        return no_enrichment_return
    all_kinds = [base_lineages[i][depth] for i in range(len(base_lineages))]
    for kind in sorted(set(all_kinds)):
        base_count = all_kinds.count(kind)
        test_count = test_kinds.count(kind)
        base_total = len(all_kinds)
        test_total = len(test_kinds)
        test_ratio = float(test_count) / test_total
        base_ratio = float(base_count) / base_total
        if test_ratio < 0.5:
            continue
        x = np.array([[test_total - test_count, test_count], [base_total - base_count, base_count]])
        if x[1, 0] == 0:
            result = (1, 1, 0, np.zeros((2, 2)))
        else:
            result = chi2_contingency_2x2(x)
        if result[1] <= 0.05 and test_ratio >= 0.5 and test_ratio > base_ratio:
            return kind, result, test_ratio
    return no_enrichment_return
