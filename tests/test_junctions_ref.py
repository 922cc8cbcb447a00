"""tests/junctions_ref.py, the plain statement of fslr_cluster_junctions, against cases worked by hand (no
device).  Every expectation below is written out as literals."""
import numpy as np

import junctions_ref as jr


def make(reads, cid=None):
    """reads: per read a list of (chrom, start, end, qkey, rev).  All reads in cluster 0 unless ``cid`` says."""
    flat = [iv for r in reads for iv in r]
    off = np.cumsum([0] + [len(r) for r in reads])
    cols = [np.asarray([iv[k] for iv in flat], np.int64) for k in range(5)]
    cid = np.zeros(len(reads), np.int64) if cid is None else np.asarray(cid, np.int64)
    return off, cols, cid, int(cid.max()) + 1


def rows_of(reads, cid=None, rev=True):
    off, (ch, s, e, key, rv), cid, nc = make(reads, cid)
    return jr.junctions(off, ch, s, e, cid, nc, key, rv if rev else None)


def as_tuples(rows):
    return [tuple(int(rows[c][k]) for c in jr.COLUMNS) for k in range(len(rows['n_obs']))]


def test_two_loci_three_reads():
    # locus 0 = [100, 210], locus 1 = [990, 1105]; every read leaves locus 0 on the right and enters locus 1 on the left
    rows = rows_of([[(0, 100, 200, 0, 0), (0, 1000, 1100, 10, 0)],
                    [(0, 110, 210, 0, 0), (0, 1005, 1105, 5, 0)],
                    [(0, 120, 190, 7, 0), (0, 990, 1090, 9, 0)]])
    assert rows['off'].tolist() == [0, 1]
    #                          la sa lb sb obs reads a_min a_max b_min b_max
    assert as_tuples(rows) == [(0, 1, 1, 0, 3, 3, 190, 210, 990, 1005)]
    assert [rows[c].dtype for c in jr.COLUMNS] == [np.int32, np.uint8, np.int32, np.uint8] + [np.int32] * 6


def test_a_read_observes_one_junction_twice_and_the_swap_carries_the_breakpoints():
    # read 0 walks locus 0 -> 1 -> 0 -> 1 (locus 0 = [100, 250], locus 1 = [1000, 1150]); read 1 has one interval
    rows = rows_of([[(0, 100, 200, 0, 0), (0, 1000, 1100, 1, 0), (0, 150, 250, 2, 0), (0, 1050, 1150, 3, 0)],
                    [(0, 120, 130, 0, 0)]])
    # the step back leaves locus 1 on the right (end 3, bp 1100) and enters locus 0 on the left (end 0, bp 150):
    # stored with end 0 first and its breakpoint 150 with it
    assert as_tuples(rows) == [(0, 0, 1, 1, 1, 1, 150, 150, 1100, 1100),
                               (0, 1, 1, 0, 2, 1, 200, 250, 1000, 1050)]
    assert int(rows['n_obs'].sum()) == 3          # L - 1 of the one read with L >= 2


def test_reverse_complement_gives_identical_rows():
    reads = [[(0, 100, 200, 0, 0), (1, 1000, 1100, 10, 1), (0, 5000, 5100, 20, 0)],
             [(0, 110, 190, 3, 1), (1, 1010, 1090, 2, 0), (0, 5010, 5090, 1, 1)],       # the same molecule, other strand
             [(1, 1020, 1030, 0, 0), (0, 105, 115, 1, 1)]]
    off, (ch, s, e, key, rv), cid, nc = make(reads)
    want = jr.junctions(off, ch, s, e, cid, nc, key, rv)
    for flipped in ([0], [1], [0, 1, 2]):
        k2, r2 = jr.reverse_complement(off, key, rv, flipped)
        got = jr.junctions(off, ch, s, e, cid, nc, k2, r2)
        for c in ('off',) + jr.COLUMNS:
            np.testing.assert_array_equal(got[c], want[c], err_msg=c)
    # loci: 0 = chrom 0 [100, 200], 1 = chrom 0 [5000, 5100], 2 = chrom 1 [1000, 1100]
    # read 0: leaves locus 0 right (1, 200), enters locus 2 right (5, 1100); leaves locus 2 left (4, 1000), enters
    # locus 1 left (2, 5000).  read 1 is its reverse complement: the same two junctions.  read 2: leaves locus 2
    # right (5, 1030), enters locus 0 right (1, 115)
    assert as_tuples(want) == [(0, 1, 2, 1, 3, 3, 115, 200, 1030, 1100),
                               (1, 0, 2, 0, 2, 2, 5000, 5010, 1000, 1010)]


def test_self_junctions_within_one_locus():
    # one locus [100, 300]; forward x then forward y: x's right end to y's left end, ea < eb
    rows = rows_of([[(0, 100, 200, 0, 0), (0, 150, 300, 1, 0)], [(0, 160, 170, 0, 0)]])
    assert as_tuples(rows) == [(0, 0, 0, 1, 1, 1, 150, 150, 200, 200)]
    # forward x, reversed y: right end to right end, ea == eb, the smaller breakpoint first
    rows = rows_of([[(0, 100, 200, 0, 0), (0, 150, 300, 1, 1)], [(0, 160, 170, 0, 0)]])
    assert as_tuples(rows) == [(0, 1, 0, 1, 1, 1, 200, 200, 300, 300)]
    # the same fold met from the other side: still (200, 300)
    rows = rows_of([[(0, 150, 300, 0, 0), (0, 100, 200, 1, 1)], [(0, 160, 170, 0, 0)]])
    assert as_tuples(rows) == [(0, 1, 0, 1, 1, 1, 200, 200, 300, 300)]


def test_key_ties_are_broken_by_csr_position():
    a, b, c = (0, 100, 200), (0, 1000, 1100), (0, 5000, 5100)           # loci 0, 1, 2
    other = [(0, 110, 120, 0, 0)]
    tied = rows_of([[a + (5, 0), b + (5, 0), c + (5, 0)], other])       # a -> b -> c
    assert as_tuples(tied) == [(0, 1, 1, 0, 1, 1, 200, 200, 1000, 1000), (1, 1, 2, 0, 1, 1, 1100, 1100, 5000, 5000)]
    early = rows_of([[a + (5, 0), b + (5, 0), c + (4, 0)], other])      # c -> a -> b
    assert as_tuples(early) == [(0, 0, 2, 1, 1, 1, 100, 100, 5100, 5100), (0, 1, 1, 0, 1, 1, 200, 200, 1000, 1000)]
    negative = rows_of([[a + (-1, 0), b + (-(1 << 31), 0), c + ((1 << 31) - 1, 0)], other])    # b -> a -> c
    assert as_tuples(negative) == [(0, 0, 1, 1, 1, 1, 100, 100, 1100, 1100), (0, 1, 2, 0, 1, 1, 200, 200, 5000, 5000)]


def test_rev_none_is_all_forward():
    reads = [[(0, 100, 200, 0, 0), (0, 1000, 1100, 1, 0)], [(0, 110, 120, 0, 0)]]
    assert as_tuples(rows_of(reads, rev=False)) == as_tuples(rows_of(reads)) == [(0, 1, 1, 0, 1, 1, 200, 200, 1000, 1000)]


def test_reads_of_one_interval_and_reads_alone_give_nothing():
    rows = rows_of([[(0, 100, 200, 0, 0)], [(0, 150, 250, 0, 0)],                     # cluster 0: one interval each
                    [(0, 100, 200, 0, 0), (0, 1000, 1100, 1, 0)]], cid=[0, 0, -1])    # a read alone with two
    assert rows['off'].tolist() == [0, 0] and all(rows[c].size == 0 for c in jr.COLUMNS)
    rows = jr.junctions([0], [], [], [], [], 0, [], [])
    assert rows['off'].tolist() == [0] and all(rows[c].size == 0 for c in jr.COLUMNS)


def test_clusters_keep_their_own_rows_and_the_observations_add_up():
    rng = np.random.default_rng(5)
    reads, cid = [], []
    for r in range(60):
        n = int(rng.integers(1, 7))
        reads.append([(int(rng.integers(0, 3)), int(s), int(s) + int(rng.integers(0, 80)), int(rng.integers(-5, 5)),
                       int(rng.integers(0, 2))) for s in rng.integers(0, 2000, n)])
        cid.append(int(rng.integers(-1, 4)))
    cid = np.asarray(cid)
    cid[:4] = [0, 1, 2, 3]
    off, (ch, s, e, key, rv), cid, nc = make(reads, cid)
    rows = jr.junctions(off, ch, s, e, cid, nc, key, rv)
    lens = np.diff(off)
    assert int(rows['n_obs'].sum()) == int((lens - 1)[(cid >= 0) & (lens >= 2)].sum())
    e_key = (rows['locus_a'].astype(np.int64) * 2 + rows['side_a']) << 32 | (rows['locus_b'].astype(np.int64) * 2 + rows['side_b'])
    assert (np.diff(e_key) > 0).all()                                   # distinct, ascending
    loci = jr.loci_ref.loci(off, ch, s, e, cid, nc)
    of_locus = np.repeat(np.arange(nc), np.diff(loci['off']))
    for c in range(nc):                                                 # both ends of a row lie in the row's cluster
        sel = slice(int(rows['off'][c]), int(rows['off'][c + 1]))
        assert (of_locus[rows['locus_a'][sel]] == c).all() and (of_locus[rows['locus_b'][sel]] == c).all()
    assert (rows['n_reads'] <= rows['n_obs']).all() and (rows['n_reads'] >= 1).all()
    assert (rows['bp_a_min'] <= rows['bp_a_max']).all() and (rows['bp_b_min'] <= rows['bp_b_max']).all()
