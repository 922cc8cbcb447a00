"""The first-fit matching of overall_jaccard_similarity (cluster.py:152-161) in plain Python: which interval
of list1 takes which interval of list2.  Test infrastructure only; not a test module.

A list is a sequence of (chrom, start, end, aln_size) in list order.  ``matching`` returns the (i, j) pairs, i
ascending, or raises ZeroDivisionError where calculate_overlap would (cluster.py:133-136: Python floats, an
aln_size of 0 on either side of a same-chromosome, not yet taken column that the walk reaches).

``prefix_matching`` derives the same thing from an overall_jaccard_similarity that keeps only the count: its
scratch marks the taken columns, and a row's choice depends on the earlier rows alone, so the column newly
marked between the calls on l1[:i] and l1[:i + 1] is row i's.
"""
import numpy as np

from fslr_amd._lib import SCORE_ZD_OVERLAP


def overlap(a, b):
    shared = max(0, min(a[2], b[2]) - max(a[1], b[1]))
    return min(shared / a[3], shared / b[3])


def matching(l1, l2, pct):
    used = [False] * len(l2)
    out = []
    for i, r in enumerate(l1):
        for j, c in enumerate(l2):
            if used[j] or r[0] != c[0]:
                continue
            if overlap(r, c) >= pct:
                used[j] = True
                out.append((i, j))
                break
    return out


def matching_or_raise(l1, l2, pct):
    """(rows, raised): the matching, or ([], True) where the reference raises."""
    try:
        return matching(l1, l2, pct), False
    except ZeroDivisionError:
        return [], True


def prefix_matching(jaccard, l1, l2, pct, scratch=None):
    """The matching by the prefix construction on ``jaccard(l1, l2, scratch, pct, min_threshold)`` (the
    reference's signature; l1, l2 lists of IntervalItem-like objects).  Raises what ``jaccard`` raises."""
    n2 = len(l2)
    scratch = np.zeros(max(n2, 1), np.int8) if scratch is None else scratch
    out = []
    before = np.zeros(n2, bool)
    for i in range(len(l1)):
        jaccard(l1[:i + 1], l2, scratch, pct, 0.5)
        now = np.asarray(scratch[:n2]) != 0
        new = np.flatnonzero(now & ~before)
        assert new.size <= 1 and not (before & ~now).any(), 'a row takes one column and keeps the earlier ones'
        if new.size:
            out.append((i, int(new[0])))
        before = now
    return out


def expect(reads, a, b, pct):
    """(offsets int64[n + 1], i int32[total], j int32[total], raised bool[n]) for the ordered pairs
    (a[k], b[k]) of ``reads`` (per read its list); each distinct pair is walked once."""
    memo = {}
    off, ii, jj, zd = [0], [], [], []
    for x, y in zip(np.asarray(a).tolist(), np.asarray(b).tolist()):
        if (x, y) not in memo:
            memo[(x, y)] = matching_or_raise(reads[x], reads[y], pct)
        rows, raised = memo[(x, y)]
        ii += [r[0] for r in rows]
        jj += [r[1] for r in rows]
        off.append(len(ii))
        zd.append(raised)
    return np.asarray(off, np.int64), np.asarray(ii, np.int32), np.asarray(jj, np.int32), np.asarray(zd, bool)


def check(got, want, I, flags):
    """``got`` = (offsets, i, j) of the device against ``want`` = expect(...), with the contract's own
    invariants: the offsets are the exclusive scan of I, a pair that raised has no rows and the flag."""
    off, gi, gj = got
    woff, wi, wj, raised = want
    np.testing.assert_array_equal(off, woff)
    np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum(I, dtype=np.int64)]))
    np.testing.assert_array_equal((np.asarray(flags) & SCORE_ZD_OVERLAP) != 0, raised)
    assert off.dtype == np.int64 and gi.dtype == np.int32 and gj.dtype == np.int32
    np.testing.assert_array_equal(gi, wi)
    np.testing.assert_array_equal(gj, wj)
