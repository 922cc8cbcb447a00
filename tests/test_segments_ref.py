"""tests/segments_ref.py, the plain statement of fslr_cluster_path_segments, against cases worked by hand (no
device).  Every expectation below is written out as literals."""
import numpy as np

import paths_ref as pr
import segments_ref as sg

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def result(reads, cid=None, qend=True):
    """reads: per read a list of (chrom, start, end, qstart, qend, rev).  All reads in cluster 0 unless ``cid`` says.
    Returns (paths, segments)."""
    flat = [iv for r in reads for iv in r]
    off = np.cumsum([0] + [len(r) for r in reads])
    ch, s, e, qs, qe, rv = (np.asarray([iv[k] for iv in flat], np.int64) for k in range(6))
    cid = np.zeros(len(reads), np.int64) if cid is None else np.asarray(cid, np.int64)
    p = pr.paths(off, ch, s, e, cid, int(cid.max()) + 1, qs, rv)
    return p, sg.segments(off, s, e, p, qs, qe if qend else None)


def cols(seg, kind):
    return [seg[f'{kind}_{w}'].tolist() for w in ('min', 'med', 'max')]


def test_the_worked_case_of_the_contract():
    # loci A = chr0:100-260 (row 0), B = chr1:500-720 (row 1); r1 is the reverse complement: B-, A- = (3, 1) > (0, 2)
    reads = [[(0, 100, 200, 0, 100, 0), (1, 500, 700, 105, 305, 0)],
             [(1, 510, 720, 0, 210, 1), (0, 120, 260, 200, 340, 1)],
             [(0, 110, 210, 0, 100, 0), (1, 505, 705, 100, 300, 0)]]
    p, seg = result(reads)
    assert pr.rows_of(p) == [((0, 2), 3, 0)] and p['flipped'].tolist() == [0, 1, 0]
    assert cols(seg, 'start') == [[100, 500], [110, 505], [120, 510]]
    assert cols(seg, 'end') == [[200, 700], [210, 705], [260, 720]]
    # gaps: r0 105 - 100 = 5, r1 200 - 210 = -10 (its own order: B first), r2 100 - 100 = 0; the last slot holds 0
    assert cols(seg, 'gap') == [[-10, 0], [0, 0], [5, 0]]
    assert all(seg[k].dtype == np.int32 and seg[k].shape == (2,) for k in sg.NAMES)


def test_lower_median_for_one_to_four_reads():
    for k, med in ((1, 10), (2, 10), (3, 20), (4, 20)):
        # k reads of one interval each on one locus, starts 10, 20, ..; ends 1000 - start
        reads = [[(0, 10 * (i + 1), 1000 - 10 * (i + 1), 0, 5, 0)] for i in range(k)]
        p, seg = result(reads + [[(0, 5000, 5001, 0, 1, 0)]], cid=[0] * k + [-1] if k > 1 else [0, 0])
        if k == 1:                                     # a cluster needs two reads: the far read is its second path
            assert pr.rows_of(p) == [((0,), 1, 0), ((2,), 1, 1)]
            assert cols(seg, 'start') == [[10, 5000]] * 3 and cols(seg, 'end') == [[990, 5001]] * 3
            continue
        assert pr.rows_of(p) == [((0,), k, 0)]
        assert cols(seg, 'start') == [[10], [med], [10 * k]]
        # the ends descend: sorted they are 1000 - 10 k .. 990, the lower median is element (k - 1) // 2
        assert cols(seg, 'end') == [[1000 - 10 * k], [sorted(1000 - 10 * (i + 1) for i in range(k))[(k - 1) // 2]], [990]]
        assert cols(seg, 'gap') == [[0], [0], [0]]
    assert sg.three([7, 3]) == (3, 3, 7) and sg.three([4, 1, 3, 2]) == (1, 2, 4) and sg.three([5]) == (5, 5, 5)


def test_a_palindromic_path_keeps_the_reads_own_order():
    # a:+ a:- (F = B = (0, 1)): not flipped, whichever way; the two reads put their first piece in slot 0
    reads = [[(0, 100, 200, 0, 50, 0), (0, 150, 250, 60, 90, 1)],
             [(0, 110, 190, 0, 40, 0), (0, 160, 240, 35, 80, 1)]]
    p, seg = result(reads)
    assert pr.rows_of(p) == [((0, 1), 2, 0)] and p['flipped'].tolist() == [0, 0]
    assert cols(seg, 'start') == [[100, 150], [100, 150], [110, 160]]
    assert cols(seg, 'end') == [[190, 240], [190, 240], [200, 250]]
    assert cols(seg, 'gap') == [[-5, 0], [-5, 0], [10, 0]]                  # 60 - 50 = 10 and 35 - 40 = -5


def test_equal_query_keys_fall_back_to_the_csr_position():
    # both intervals of each read have key 7: the chain is the CSR order, the gap is 7 - qend of the first
    reads = [[(0, 100, 200, 7, 9, 0), (0, 5000, 5100, 7, 30, 0)],
             [(0, 120, 220, 7, 2, 0), (0, 5010, 5110, 7, 8, 0)]]
    p, seg = result(reads)
    assert pr.rows_of(p) == [((0, 2), 2, 0)]
    assert cols(seg, 'start') == [[100, 5000], [100, 5000], [120, 5010]]
    assert cols(seg, 'gap') == [[-2, 0], [-2, 0], [5, 0]]


def test_without_qend_every_gap_is_zero():
    reads = [[(0, 100, 200, 0, 100, 0), (1, 500, 700, 105, 305, 0)], [(0, 110, 210, 0, 100, 0), (1, 505, 705, 100, 300, 0)]]
    _, seg = result(reads, qend=False)
    assert cols(seg, 'gap') == [[0, 0]] * 3 and cols(seg, 'start') == [[100, 500], [100, 500], [110, 505]]


def test_gaps_saturate_at_both_ends_of_int32():
    # next key I32_MAX minus qend -1 = 2^31 -> I32_MAX; next key I32_MIN + 1 ... the chain order is by key, so the
    # low side is reached with a large qend: key 0 then key 1, 1 - I32_MAX = I32_MIN + 2; with qend I32_MAX and a
    # negative next key the difference passes the low end
    reads = [[(0, 100, 200, -5, -1, 0), (0, 5000, 5100, I32_MAX, I32_MAX, 0)],
             [(0, 110, 210, I32_MIN, I32_MAX, 0), (0, 5010, 5110, -2, 0, 0)]]
    p, seg = result(reads)
    assert pr.rows_of(p) == [((0, 2), 2, 0)]
    # read 0: I32_MAX - (-1) = 2^31 -> I32_MAX; read 1: -2 - I32_MAX = -2^31 - 1 -> I32_MIN
    assert cols(seg, 'gap') == [[I32_MIN, 0], [I32_MIN, 0], [I32_MAX, 0]]


def test_several_rows_and_an_unclustered_read():
    # cluster 0: two reads (A, C) and one read (A) alone on its path; read 3 is not clustered
    reads = [[(0, 100, 200, 0, 10, 0), (0, 5000, 5100, 12, 20, 0)],
             [(0, 105, 190, 0, 10, 0), (0, 5005, 5090, 9, 20, 0)],
             [(0, 150, 160, 0, 10, 0)],
             [(0, 9000, 9100, 0, 10, 0)]]
    p, seg = result(reads, cid=[0, 0, 0, -1])
    assert pr.rows_of(p) == [((0,), 1, 2), ((0, 2), 2, 0)] and p['tok_off'].tolist() == [0, 1, 3]
    assert cols(seg, 'start') == [[150, 100, 5000], [150, 100, 5000], [150, 105, 5005]]
    assert cols(seg, 'end') == [[160, 190, 5090], [160, 190, 5090], [160, 200, 5100]]
    assert cols(seg, 'gap') == [[0, -1, 0], [0, -1, 0], [0, 2, 0]]
