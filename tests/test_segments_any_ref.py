"""tests/segments_ref.py, the plain statement of the path segments, beyond 64 intervals: one hand-worked read of 65
intervals and its reverse complement (no device).  fslr_cluster_path_segments_any is compared against this
statement, so the statement itself is pinned where a read crosses the chunk seam.  Every expectation is written out
as literals or as a closed form of the slot number."""
import numpy as np

import paths_ref as pr
import segments_ref as sg

L = 65


def two_reads(equal_keys=False):
    """Read A walks loci 0..64 forward: piece t = chr0:1000 t..1000 t + 100, query 10 t..10 t + 7, but piece 63 ends at
    query 642.  Read B is the same molecule from the other strand: every piece reversed, 5 bases to the right, and the
    piece on locus t has chain rank u = 64 - t: query 10 u..10 u + 6, but rank 0 ends at 15 and rank 63 at 631.  Both
    lists stand in locus order, so B's list positions 63 and 64, the two sides of its chunk seam, are its chain
    ranks 1 and 0."""
    a = [(0, 1000 * t, 1000 * t + 100, 10 * t, 642 if t == 63 else 10 * t + 7, 0) for t in range(L)]
    b = []
    for t in range(L):
        u = L - 1 - t
        b.append((0, 1000 * t + 5, 1000 * t + 105, 10 * u, {0: 15, 63: 631}.get(u, 10 * u + 6), 1))
    if equal_keys:                                  # every key 7: the chain is the list order, B walks forward too
        a = [(c, s, e, 7, qe, 0) for c, s, e, _, qe, _ in a]
        b = [(c, s, e, 7, qe, 0) for c, s, e, _, qe, _ in b]
    flat = a + b
    ch, s, e, qs, qe, rv = (np.asarray([iv[k] for iv in flat], np.int64) for k in range(6))
    off = np.asarray([0, L, 2 * L])
    p = pr.paths(off, ch, s, e, np.zeros(2, np.int64), 1, qs, rv)
    return p, sg.segments(off, s, e, p, qs, qe)


def test_a_read_of_65_intervals_and_its_reverse_complement_share_every_slot():
    p, seg = two_reads()
    # one row of 65 tokens, locus t forward at position t; A stands as it is, B is flipped
    assert pr.rows_of(p) == [(tuple(range(0, 2 * L, 2)), 2, 0)]
    assert p['flipped'].tolist() == [0, 1] and p['tok_off'].tolist() == [0, L]
    t = np.arange(L)
    assert seg['start_min'].tolist() == seg['start_med'].tolist() == (1000 * t).tolist()
    assert seg['start_max'].tolist() == (1000 * t + 5).tolist()
    assert seg['end_min'].tolist() == seg['end_med'].tolist() == (1000 * t + 100).tolist()
    assert seg['end_max'].tolist() == (1000 * t + 105).tolist()
    # links 1..62: A leaves 10 (t + 1) - (10 t + 7) = 3, B leaves 10 (u + 1) - (10 u + 6) = 4 on the same link
    assert seg['gap_min'][1:63].tolist() == seg['gap_med'][1:63].tolist() == [3] * 62
    assert seg['gap_max'][1:63].tolist() == [4] * 62
    # link 0: A 10 - 7 = 3; B's ranks 63 -> 64: 640 - 631 = 9
    assert [seg[k][0] for k in sg.NAMES[6:]] == [3, 3, 9]
    # link 63, the chunk seam of both lists and the last link (L - 2): A 640 - 642 = -2; B's ranks 0 -> 1: 10 - 15 = -5
    assert [seg[k][63] for k in sg.NAMES[6:]] == [-5, -5, -2]
    # the last slot holds no gap
    assert [seg[k][64] for k in sg.NAMES[6:]] == [0, 0, 0]
    assert all(seg[k].dtype == np.int32 and seg[k].shape == (L,) for k in sg.NAMES)


def test_equal_keys_across_the_seam_keep_the_list_order():
    p, seg = two_reads(equal_keys=True)
    assert pr.rows_of(p) == [(tuple(range(0, 2 * L, 2)), 2, 0)] and p['flipped'].tolist() == [0, 0]
    # the gap at link t is 7 - qend of list position t: A 7 - (10 t + 7) = -10 t, but 7 - 642 = -635 at 63;
    # B's position t has rank u = 64 - t: 7 - (10 u + 6) = 1 - 10 u, but 7 - 631 = -624 at t = 1 (u = 63)
    a = [-10 * t for t in range(L - 1)]
    a[63] = -635
    b = [1 - 10 * (L - 1 - t) for t in range(L - 1)]
    b[1] = -624
    assert seg['gap_min'][:-1].tolist() == seg['gap_med'][:-1].tolist() == [min(x, y) for x, y in zip(a, b)]
    assert seg['gap_max'][:-1].tolist() == [max(x, y) for x, y in zip(a, b)]
    assert [seg[k][63] for k in sg.NAMES[6:]] == [-635, -635, -9] and [seg[k][64] for k in sg.NAMES[6:]] == [0, 0, 0]
