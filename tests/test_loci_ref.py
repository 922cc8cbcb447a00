"""tests/loci_ref.py against hand-worked cases and against a second statement of the definition: per-position
coverage over a small coordinate range (no device)."""
import numpy as np
import pytest

import loci_ref as lr


def run(reads, cid, n_clusters):
    """reads: per read a list of (chrom, start, end)."""
    off = np.cumsum([0] + [len(r) for r in reads])
    flat = [iv for r in reads for iv in r]
    col = lambda k: np.asarray([iv[k] for iv in flat], np.int64)
    return lr.loci(off, col(0), col(1), col(2), np.asarray(cid), n_clusters)


def rows_of(out):
    return list(zip(*(out[c].tolist() for c in lr.COLUMNS)))


def test_nested_intervals_make_one_locus_with_the_largest_end():
    out = run([[(0, 10, 100)], [(0, 20, 30)], [(0, 40, 50), (0, 95, 99)]], [0, 0, 0], 1)
    assert rows_of(out) == [(0, 10, 100, 4, 3)]
    assert out['off'].tolist() == [0, 1]


def test_the_running_maximum_decides_not_the_last_end():
    # 60 > 30 (the previous interval's end) but 60 <= 100 (the largest so far)
    out = run([[(0, 10, 100)], [(0, 20, 30)], [(0, 60, 70)], [(0, 101, 110)]], [0, 0, 0, 0], 1)
    assert rows_of(out) == [(0, 10, 100, 3, 3), (0, 101, 110, 1, 1)]


def test_touching_merges_and_one_past_does_not():
    out = run([[(0, 10, 20)], [(0, 20, 30)], [(0, 31, 40)]], [0, 0, 0], 1)
    assert rows_of(out) == [(0, 10, 30, 2, 2), (0, 31, 40, 1, 1)]


def test_equal_starts_in_any_order():
    a = run([[(0, 5, 9)], [(0, 5, 50)], [(0, 5, 7)], [(0, 51, 60)]], [0, 0, 0, 0], 1)
    b = run([[(0, 5, 50)], [(0, 5, 7)], [(0, 51, 60)], [(0, 5, 9)]], [0, 0, 0, 0], 1)
    assert rows_of(a) == rows_of(b) == [(0, 5, 50, 3, 3), (0, 51, 60, 1, 1)]


def test_a_read_counts_once_per_locus():
    # read 0: three intervals in the first locus and one in the second locus of chromosome 0, one on chromosome 1
    r0 = [(0, 10, 20), (0, 15, 25), (0, 22, 30), (0, 100, 110), (1, 5, 6)]
    r1 = [(0, 12, 14), (0, 105, 120)]
    out = run([r0, r1], [0, 0], 1)
    assert rows_of(out) == [(0, 10, 30, 4, 2), (0, 100, 120, 2, 2), (1, 5, 6, 1, 1)]


def test_clusters_chromosomes_and_reads_alone():
    reads = [[(1, 10, 20)], [(0, 10, 20)], [(0, 5, 8)], [(1, 15, 30), (0, 1, 2)], [(0, 0, 1000)], [(0, 7, 9)]]
    out = run(reads, [1, 0, 0, 1, -1, 0], 2)
    assert rows_of(out) == [(0, 5, 9, 2, 2), (0, 10, 20, 1, 1), (0, 1, 2, 1, 1), (1, 10, 30, 2, 2)]
    assert out['off'].tolist() == [0, 2, 4]


def test_no_clusters():
    out = run([[(0, 1, 2)], [(0, 1, 2)]], [-1, -1], 0)
    assert out['off'].tolist() == [0] and all(out[c].size == 0 and out[c].dtype == np.int32 for c in lr.COLUMNS)


def test_cids_of_labels():
    cid, nc = lr.cids_of_labels([0, 1, 0, 3, 1, 5])
    assert cid.tolist() == [0, 1, 0, -1, 1, -1] and nc == 2
    assert lr.cids_of_labels(np.zeros(0, np.int32))[1] == 0


# ---- the second statement: coverage per position -------------------------------------------------
def brute(reads, cid, n_clusters, n_chroms, span):
    """Positions s .. e of an interval are covered, and x, x + 1 are linked when one interval covers both; a
    locus is a maximal run of covered positions joined by links."""
    rows, off = [], [0]
    for c in range(n_clusters):
        for ch in range(n_chroms):
            ivs = [(s, e, r) for r, lst in enumerate(reads) if cid[r] == c for (h, s, e) in lst if h == ch]
            cov, link = np.zeros(span, bool), np.zeros(span, bool)
            for s, e, _ in ivs:
                cov[s:e + 1] = True
                link[s:e] = True                      # x -> x + 1 for x in [s, e)
            x = 0
            while x < span:
                if not cov[x]:
                    x += 1
                    continue
                y = x
                while link[y]:
                    y += 1
                inside = [(s, r) for s, e, r in ivs if x <= s <= y]
                rows.append((ch, x, y, len(inside), len({r for _, r in inside})))
                x = y + 1
        off.append(len(rows))
    return rows, off


@pytest.mark.parametrize('seed', range(12))
def test_against_the_coverage_statement(seed):
    rng = np.random.default_rng(seed)
    span, n_chroms = 60, 3
    n_reads = int(rng.integers(2, 40))
    reads = []
    for _ in range(n_reads):
        lst = []
        for _ in range(int(rng.integers(1, 5))):
            s = int(rng.integers(0, span))
            e = min(span - 1, s + int(rng.integers(0, 6 if seed % 2 else 15)))
            lst.append((int(rng.integers(0, n_chroms)), s, e))
        reads.append(lst)
    n_clusters = int(rng.integers(0, 5))
    cid = rng.integers(-1, n_clusters, n_reads) if n_clusters else np.full(n_reads, -1)
    out = run(reads, cid, n_clusters)
    want, off = brute(reads, cid, n_clusters, n_chroms, span)
    assert rows_of(out) == want
    assert out['off'].tolist() == off


def test_bed_text():
    out = run([[(1, 10, 20)], [(1, 20, 25), (0, 3, 4)]], [0, 0], 1)
    assert lr.bed_text(out, ['chrA', 'chrB']) == ('cluster\tchrom\tstart\tend\tn_intervals\tn_reads\n'
                                                  '0\tchrA\t3\t4\t1\t1\n0\tchrB\t10\t25\t2\t2\n')
