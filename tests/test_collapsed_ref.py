"""tests/collapsed_ref.py, the plain statement of the collapsed path segments, pinned on hand-worked clusters (no
device).  fslr_cluster_collapsed_segments is compared against this statement.  Every expectation is written out as
literals or as a closed form of the slot number."""
import numpy as np

import collapsed_ref as cl
import containment_ref as cr
import paths_ref as pr

GAPS = cl.NAMES[8:]


def run(reads, with_qend=True):
    """``reads``: lists of (start, end, query start, query end, rev) on chromosome 0, one cluster."""
    flat = [iv for r in reads for iv in r]
    s, e, qs, qe, rv = (np.asarray([iv[k] for iv in flat], np.int64) for k in range(5))
    off = np.cumsum([0] + [len(r) for r in reads])
    p = pr.paths(off, np.zeros(len(flat), np.int64), s, e, np.zeros(len(reads), np.int64), 1, qs, rv)
    ct = cr.containment(p)
    return p, ct, cl.collapsed(off, s, e, p, ct, qs, qe if with_qend else None)


def three_loci():
    r0 = [(0, 100, 0, 10, 0), (10000, 10100, 12, 20, 0), (20000, 20100, 25, 30, 0)]        # gaps 2, 5
    r1 = [(2, 102, 0, 9, 0), (10002, 10102, 13, 21, 0), (20002, 20102, 24, 31, 0)]        # gaps 4, 3
    r2 = [(10004, 10104, 0, 8, 0), (20004, 20104, 9, 15, 0)]                              # gap 1
    r3 = [(6, 106, 13, 20, 1), (10006, 10106, 0, 7, 1)]       # walks L1-, L0-: the gap 13 - 7 = 6
    return [r0, r1, r2, r3]


def test_truncated_reads_count_at_the_pieces_they_cover():
    p, ct, got = run(three_loci())
    # rows ascend: (L0+, L1+) of r3 flipped, (L0+, L1+, L2+) of r0 and r1, (L1+, L2+) of r2
    assert pr.rows_of(p) == [((0, 2), 1, 3), ((0, 2, 4), 2, 0), ((2, 4), 1, 2)]
    assert p['flipped'].tolist() == [0, 0, 0, 1] and p['tok_off'].tolist() == [0, 2, 5, 7]
    assert ct['collapse_to'].tolist() == [1, 1, 1] and ct['offset'].tolist() == [0, 1] and ct['rev'].tolist() == [0, 0]
    assert got['n_cov'].tolist() == [0, 0, 3, 4, 3, 0, 0]
    assert got['n_link'].tolist() == [0, 0, 3, 3, 0, 0, 0]
    assert got['start_min'].tolist() == [0, 0, 0, 10000, 20000, 0, 0]
    assert got['start_med'].tolist() == [0, 0, 2, 10002, 20002, 0, 0]
    assert got['start_max'].tolist() == [0, 0, 6, 10006, 20004, 0, 0]
    assert got['end_min'].tolist() == [0, 0, 100, 10100, 20100, 0, 0]
    assert got['end_med'].tolist() == [0, 0, 102, 10102, 20102, 0, 0]
    assert got['end_max'].tolist() == [0, 0, 106, 10106, 20104, 0, 0]
    # the first link: r0 2, r1 4 and r3 6, positive as when its molecule is read forwards; the second: 5, 3 and r2's 1
    assert got['gap_min'].tolist() == [0, 0, 2, 1, 0, 0, 0]
    assert got['gap_med'].tolist() == [0, 0, 4, 3, 0, 0, 0]
    assert got['gap_max'].tolist() == [0, 0, 6, 5, 0, 0, 0]
    assert all(got[k].dtype == np.int32 and got[k].shape == (7,) for k in cl.NAMES)


def test_without_query_ends_the_links_are_still_counted():
    _, _, got = run(three_loci(), with_qend=False)
    assert got['n_link'].tolist() == [0, 0, 3, 3, 0, 0, 0] and got['n_cov'].tolist() == [0, 0, 3, 4, 3, 0, 0]
    assert all(got[k].tolist() == [0] * 7 for k in GAPS)
    assert got['start_med'].tolist() == [0, 0, 2, 10002, 20002, 0, 0]


def test_a_short_row_stored_as_the_reverse_complement_of_the_outers_sub_chain():
    y = [(0, 100, 0, 10, 0), (20000, 20100, 14, 20, 1), (10000, 10100, 21, 30, 1)]        # L0+, L2-, L1-: gaps 4, 1
    x = [(10004, 10104, 0, 8, 0), (20004, 20104, 11, 15, 0)]                              # L1+, L2+: gap 3
    p, ct, got = run([y, x])
    assert pr.rows_of(p) == [((0, 5, 3), 1, 0), ((2, 4), 1, 1)] and p['flipped'].tolist() == [0, 0]
    assert ct['collapse_to'].tolist() == [0, 0] and ct['offset'].tolist() == [1] and ct['rev'].tolist() == [1]
    # x's L1 piece lands at the outer's position 2 and its L2 piece at position 1; its link at position 1
    assert got['n_cov'].tolist() == [1, 2, 2, 0, 0] and got['n_link'].tolist() == [1, 2, 0, 0, 0]
    assert [got[k].tolist() for k in cl.NAMES[2:5]] == [[0, 20000, 10000, 0, 0], [0, 20000, 10000, 0, 0], [0, 20004, 10004, 0, 0]]
    assert [got[k].tolist() for k in cl.NAMES[5:8]] == [[100, 20100, 10100, 0, 0], [100, 20100, 10100, 0, 0], [100, 20104, 10104, 0, 0]]
    assert [got[k].tolist() for k in GAPS] == [[4, 1, 0, 0, 0], [4, 1, 0, 0, 0], [4, 3, 0, 0, 0]]


def test_a_read_of_65_intervals_collapses_onto_one_of_66():
    """The outer walks loci 0..65: piece t = 1000 t..1000 t + 100, query 10 t..10 t + 7.  The inner walks loci 1..65:
    the piece on locus t is 5 bases to the right and has chain rank u = t - 1, query 10 u..10 u + 6.  Its list
    positions 63 and 64, the two sides of its chunk seam, are the loci 64 and 65."""
    outer = [(1000 * t, 1000 * t + 100, 10 * t, 10 * t + 7, 0) for t in range(66)]
    inner = [(1000 * t + 5, 1000 * t + 105, 10 * (t - 1), 10 * (t - 1) + 6, 0) for t in range(1, 66)]
    p, ct, got = run([outer, inner])
    assert p['tok_off'].tolist() == [0, 66, 131] and ct['collapse_to'].tolist() == [0, 0]
    assert ct['offset'].tolist() == [1] and ct['rev'].tolist() == [0]
    t = np.arange(66)
    assert got['n_cov'].tolist() == [1] + [2] * 65 + [0] * 65
    assert got['n_link'].tolist() == [1] + [2] * 64 + [0] + [0] * 65
    assert got['start_min'][:66].tolist() == got['start_med'][:66].tolist() == (1000 * t).tolist()
    assert got['start_max'][:66].tolist() == [0] + (1000 * t[1:] + 5).tolist()
    assert got['end_max'][:66].tolist() == [100] + (1000 * t[1:] + 105).tolist()
    # the outer leaves 10 (t + 1) - (10 t + 7) = 3 on every link, the inner 10 (u + 1) - (10 u + 6) = 4 on the links 1..64,
    # the one between its list positions 63 and 64 (slot 64) among them
    assert got['gap_min'][:66].tolist() == got['gap_med'][:66].tolist() == [3] * 65 + [0]
    assert got['gap_max'][:66].tolist() == [3] + [4] * 64 + [0]
    assert all(not got[k][66:].any() for k in cl.NAMES)
