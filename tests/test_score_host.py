"""The host drop-ins of the reference's pair predicates (cluster.py:133-183) against its own known
answers (tests/golden/kats.json.gz): calculate_overlap, overall_jaccard_similarity,
different_lengths_or_alignments with IntervalItem arguments, float equality included."""
import numpy as np
import pytest

import fixtures as fx
from fslr_amd import cluster
from fslr_amd.prep import IntervalItem


def item(chrom, start, end, aln, qname='q', nal=1, qlen2=1, index=0):
    return IntervalItem(chrom, start, end, aln, qname, nal, qlen2, start + aln // 2, index)


def items(lst):
    return [item(*t) for t in lst]


def test_exported():
    for name in ('calculate_overlap', 'overall_jaccard_similarity', 'different_lengths_or_alignments'):
        assert name in cluster.__all__ and callable(getattr(cluster, name))


def test_kat_overlap():
    kats = fx.kats()['overlap']
    assert len(kats) == 3000
    for k in kats:
        r = cluster.calculate_overlap(item(1, 0, k['o'], k['a1']), item(1, 0, k['end2'], k['a2']))
        assert isinstance(r, float)
        assert r == min(k['o'] / k['a1'], k['o'] / k['a2'])
        assert (r >= k['pct']) == k['ok'], k


def test_overlap_values_and_zero_division():
    assert cluster.calculate_overlap(item(1, 0, 100, 50), item(1, 200, 300, 50)) == 0.0     # disjoint: never below 0
    assert cluster.calculate_overlap(item(1, 0, 100, 50), item(1, 40, 300, 200)) == 0.3
    with pytest.raises(ZeroDivisionError):
        cluster.calculate_overlap(item(1, 0, 100, 0), item(1, 200, 300, 50))                # even where nothing is shared
    with pytest.raises(ZeroDivisionError):
        cluster.calculate_overlap(item(1, 0, 100, 50), item(1, 0, 100, 0))


def test_kat_lengths():
    kats = fx.kats()['lengths']
    assert len(kats) == 3007
    for k in kats:
        a, b = item(1, 0, 1, 1, nal=k['n1'], qlen2=k['q1']), item(1, 0, 1, 1, nal=k['n2'], qlen2=k['q2'])
        if 'raises' in k:
            with pytest.raises(ZeroDivisionError):
                cluster.different_lengths_or_alignments(a, b, k['qd'], k['nd'])
        else:
            assert cluster.different_lengths_or_alignments(a, b, k['qd'], k['nd']) is k['differ'], k


def test_kat_jaccard():
    kats = fx.kats()['jaccard']
    assert len(kats) == 3005
    scratch = np.zeros(100000)
    for k in kats:
        a, b = items(k['a']), items(k['b'])
        if 'raises' in k:
            with pytest.raises(ZeroDivisionError):
                cluster.overall_jaccard_similarity(a, b, scratch, k['pct'], 0.5)
            continue
        j, n_i = cluster.overall_jaccard_similarity(a, b, scratch, k['pct'], 0.5)
        assert (j, n_i) == (k['j'], k['n_i']), k
        assert type(n_i) is int


def test_scratch_is_mutated_as_the_reference_leaves_it():
    a = items([(1, 0, 100, 100), (1, 500, 600, 100), (2, 0, 100, 100)])
    b = items([(2, 0, 100, 100), (1, 0, 100, 100), (1, 900, 990, 90), (1, 500, 600, 100)])
    scratch = np.full(8, 7.0)
    j, n_i = cluster.overall_jaccard_similarity(a, b, scratch, 0.8, 0.5)
    assert (j, n_i) == (3 / 4, 3)
    # the first len(l2) entries: cleared, then 1 at the columns taken; the rest untouched
    np.testing.assert_array_equal(scratch, [1, 1, 0, 1, 7, 7, 7, 7])
    # a column taken by an earlier row is not offered again: two equal rows, one column
    two = items([(1, 0, 100, 100), (1, 0, 100, 100)])
    assert cluster.overall_jaccard_similarity(two, two[:1], scratch, 0.8, 0.5) == (1 / 2, 1)
    np.testing.assert_array_equal(scratch, [1, 1, 0, 1, 7, 7, 7, 7])
    # min_threshold has no effect
    assert cluster.overall_jaccard_similarity(a, b, scratch, 0.8, 0.0) == (3 / 4, 3)
    assert cluster.overall_jaccard_similarity(a, b, scratch, 0.8, 1.0) == (3 / 4, 3)


def test_empty_lists():
    a = items([(1, 0, 100, 100)])
    scratch = np.full(4, 5.0)
    for l1, l2 in (([], a), (a, []), ([], [])):
        r = cluster.overall_jaccard_similarity(l1, l2, scratch, 0.8, 0.5)
        assert r == (0, 0) and all(type(x) is int for x in r)
    np.testing.assert_array_equal(scratch, [5, 5, 5, 5])                # returned before the scratch is touched
