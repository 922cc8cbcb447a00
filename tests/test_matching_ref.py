"""tests/matching_ref.py (the plain statement of the first-fit matching) against the prefix construction on
the host drop-in of overall_jaccard_similarity (whose scratch behaves as the reference's, test_score_host.py),
the C oracle's count, the reference's Jaccard known answers and the fixture recorded from the reference
itself (tests/golden/matching/pairs.npz).  No device."""
import os

import numpy as np
import pytest

import fixtures as fx
import host_pipeline as hp
import matching_ref as mr
from fslr_amd import cluster
from fslr_amd.prep import IntervalItem
from oracle import oracle as O

FIXTURE = os.path.join(fx.GOLDEN, 'matching', 'pairs.npz')


def items(lst):
    return [IntervalItem(c, s, e, a, 'q', 1, 1, s + a // 2, 0) for c, s, e, a in lst]


def by_prefix(l1, l2, pct):
    try:
        return mr.prefix_matching(cluster.overall_jaccard_similarity, items(l1), items(l2), pct), False
    except ZeroDivisionError:
        return [], True


def test_kats_prefix_construction_and_count():
    """Every Jaccard KAT, both orientations: the plain statement == the prefix construction; its length is the
    KAT's n_i and the oracle's I; a raise is a raise in all three."""
    kats = fx.kats()['jaccard']
    raised = nonzero = 0
    for t, k in enumerate(kats):
        for l1, l2 in ((k['a'], k['b']), (k['b'], k['a'])):
            if not l1 or not l2:
                continue
            rows, zd = mr.matching_or_raise(l1, l2, k['pct'])
            if t % 4 == 0 or zd:
                assert by_prefix(l1, l2, k['pct']) == (rows, zd), (t, k)
            try:
                I, U = O.jaccard_lists(l1, l2, k['pct'])
                assert not zd and (I, U) == (len(rows), len(l1) + len(l2) - len(rows)), (t, k)
            except ZeroDivisionError:
                assert zd, (t, k)
        rows, zd = mr.matching_or_raise(k['a'], k['b'], k['pct']) if k['a'] and k['b'] else ([], False)
        if 'raises' in k:
            assert zd, (t, k)
            raised += 1
        elif not zd:
            assert len(rows) == k['n_i'], (t, k)
            nonzero += k['n_i'] > 0
    assert raised >= 1 and nonzero > 100


def test_shape_of_a_matching():
    X = (1, 1000, 2000, 1000)
    far = (1, 50_000, 51_000, 1000)
    other = (2, 1000, 2000, 1000)
    # row 0 takes column 2 (the first on its chromosome that matches), row 1 column 0
    assert mr.matching([X, other], [other, far, X], 0.8) == [(0, 2), (1, 0)]
    # an unmatched row between matched ones; a taken column that a later row would also match
    assert mr.matching([X, far, X, X], [X, X], 0.8) == [(0, 0), (2, 1)]
    assert mr.matching([X, X, X], [X], 0.8) == [(0, 0)]
    # rows ascend, columns are distinct
    assert mr.matching([far, X], [X, far], 0.8) == [(0, 1), (1, 0)]
    # the raise: an aln_size == 0 column on the row's chromosome, reached before a match; not reached behind one
    Z = (1, 1000, 2000, 0)
    with pytest.raises(ZeroDivisionError):
        mr.matching([X], [Z, X], 0.8)
    assert mr.matching([X], [X, Z], 0.8) == [(0, 0)]
    assert mr.matching([X], [(2, 1000, 2000, 0), X], 0.8) == [(0, 1)]
    with pytest.raises(ZeroDivisionError):          # after two matches
        mr.matching([X, X, X], [X, X, Z], 0.8)
    assert by_prefix([X, X, X], [X, X, Z], 0.8) == ([], True)
    assert by_prefix([X, far, X, X], [X, X], 0.8) == ([(0, 0), (2, 1)], False)


def fixture_sources():
    z = np.load(FIXTURE)
    return z, z['sources'].tolist()


def lists_of(name):
    data, _, _ = hp.host_prepare(name)
    csr = data.csr()
    dp = np.asarray(csr.data_pos, np.int64)
    return [list(zip(*(getattr(data, f)[dp[csr.read_off[r]:csr.read_off[r + 1]]].tolist()
                       for f in ('chrom', 'start', 'end', 'aln_size')))) for r in range(csr.n_reads)]


def test_recorded_from_the_reference():
    """The fixture holds what the reference did; the plain statement reproduces it on the same inputs."""
    z, sources = fixture_sources()
    total = raised = empty = skipped = 0
    for name in sources:
        reads = lists_of(name)
        a, b = z[f'{name}_a'], z[f'{name}_b']
        off, i, j, zd = mr.expect(reads, a, b, float(z[f'{name}_pct']))
        np.testing.assert_array_equal(off, z[f'{name}_off'])
        np.testing.assert_array_equal(i, z[f'{name}_i'])
        np.testing.assert_array_equal(j, z[f'{name}_j'])
        np.testing.assert_array_equal(zd, z[f'{name}_raised'])
        total += a.size
        raised += int(zd.sum())
        empty += int(((np.diff(off) == 0) & ~zd).sum())
        for k in range(a.size):
            cols = j[off[k]:off[k + 1]].tolist()
            skipped += any(any(c not in cols[:m] for c in range(x)) for m, x in enumerate(cols))
    assert 250 <= total <= 400 and raised >= 3 and empty >= 3 and skipped >= 3
