"""Host side of pair scoring for reads of any length (fslr_score_pairs_any): the exported symbol, the
reference of tests/any_ref.py against the plain first-fit of tests/long_ref.py and the C oracle on the
directed inputs, and the argument checks of the Python layer, which need no device."""
import ctypes

import numpy as np
import pytest

import any_ref as ar
import long_ref as lr
import search_ref as sr
from any_ref import X, Z, diag, filler, with_at
from fslr_amd import _lib, cluster
from fslr_amd._lib import SCORE_EDGE, SCORE_GATE, SCORE_ZD_GATE, SCORE_ZD_OVERLAP
from fslr_amd.prep import fold_overlap_threshold, pass_table, umax_table


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def test_symbol_rejects_a_null_context(lib):
    assert 'fslr_score_pairs_any' in _lib.EXPORTED and hasattr(lib, 'fslr_score_pairs_any')
    out = np.full(3, -7, np.int32)
    rc = lib.fslr_score_pairs_any(None, None, None, 0, 3, None, None, out.ctypes.data_as(ctypes.c_void_p), None, None)
    assert rc == _lib.FSLR_ERR_INVALID and (out == -7).all()
    for name in ('fslr_match_reads_any', 'fslr_match_rows_any'):
        assert name in _lib.EXPORTED and hasattr(lib, name), name
    total = ctypes.c_int64(-1)
    assert lib.fslr_match_reads_any(None, None, None, 0, None, 0, None, None, None, ctypes.byref(total)) == \
        _lib.FSLR_ERR_INVALID
    assert lib.fslr_match_rows_any(None, None, None, None, None, 0) == _lib.FSLR_ERR_INVALID
    assert total.value == -1


def test_reference_agrees_with_the_plain_first_fit():
    """any_ref.fit (the C oracle) against long_ref.first_fit (plain Python, from the reference's lines) on the
    directed lists, in both orientations."""
    cases = [(diag(65), diag(64)), (diag(129), diag(130)), (with_at(70, 2, {0: X, 1: X}), with_at(140, 3, {0: X, 130: X})),
             (with_at(140, 2, {130: X}), with_at(70, 3, {0: X})), ([X] * 130, [X] * 67)]
    for name, (la, lb, places) in lr.GADGET_PLACES.items():
        for swap in (False, True):
            data = lr.gadgets(la, lb, places, swap)
            rank, lists = lr.rank_of(data), lr.read_lists(data.csr())
            cases.append((lists[rank[0]], lists[rank[1]]))
    for l1, l2 in cases:
        for x, y in ((l1, l2), (l2, l1)):
            I, U, zd = ar.fit(x, y, 0.5)
            assert not zd and I == lr.first_fit(x, y, 0.5) and U == len(x) + len(y) - I
    assert ar.fit([X], with_at(140, 3, {70: Z, 130: X}), 0.5) == (0, 0, True)
    assert ar.fit([X], with_at(140, 3, {130: X, 135: Z}), 0.5) == (1, 140, False)
    assert ar.fit([X], with_at(140, 3, {70: (5, 1000, 2000, 0), 130: X}), 0.5) == (1, 140, False)
    assert ar.fit([Z], [X], 0.5) == (0, 0, True)


def test_flag_byte_and_cutoff_tables():
    """The float rule of any_ref.flag_byte is the pass table inside the table and umax_table beyond it."""
    for cuts in (ar.CUTS, [0.5], [0.07], [0.001, 0.001, 0.5]):
        pt = pass_table(cuts).reshape(-1, _lib.PASS_STRIDE)
        um = umax_table(cuts, 4096)
        for I, U in [(1, 1), (6, 12), (6, 13), (64, 128), (10, 128)]:
            assert bool(ar.flag_byte(I, U, False, 9, 9, 3, 3, cuts) & SCORE_EDGE) == bool(pt[I - 1, U - 1]), (cuts, I, U)
        for I, U in [(65, 130), (65, 131), (10, 129), (6, 130), (1, 130), (1, 8191), (4096, 4096), (257, 300)]:
            assert bool(ar.flag_byte(I, U, False, 9, 9, 3, 3, cuts) & SCORE_EDGE) == (U <= um[I - 1]), (cuts, I, U)
    assert ar.flag_byte(0, 0, True, 9, 9, 3, 3, ar.CUTS) == SCORE_GATE | SCORE_ZD_OVERLAP
    assert ar.flag_byte(129, 130, False, 0, 0, 3, 3, ar.CUTS) == SCORE_ZD_GATE
    assert ar.flag_byte(130, 130, False, 500, 1000, 2, 4, ar.CUTS) == 0
    thr = fold_overlap_threshold(np.array([1000, 0]), 0.5)
    assert thr[1] == _lib.FSLR_THR_ZERO_ALN and thr[0] != _lib.FSLR_THR_ZERO_ALN


def test_pool_csr():
    p = ar.Pool(0.5)
    p.add(diag(3))
    p.add(filler(70, 2), qlen2=7, nal=2)
    c = p.csr()
    assert c.read_off.tolist() == [0, 3, 73] and c.n_chroms == 3 and c.read_qlen2.tolist() == [ar.QLEN2, 7]
    assert p.max_len() == 70 and not c.start_sorted
    I, U, F = p.expect([0, 0], [0, 1], ar.CUTS)
    assert I.tolist() == [3, 0] and U.tolist() == [3, 73] and F[0] == SCORE_GATE | SCORE_EDGE and F[1] == 0


class _NoDevice:
    """A context that must not be reached: the Python layer refuses the call first."""

    def __getattr__(self, name):
        raise AssertionError(f'the device was asked for {name}')


def test_python_layer_argument_checks():
    data = sr.make_data([5, 2, 9, 2], [10, 20, 30, 40], [15, 25, 35, 45])
    idx = object.__new__(cluster.DeviceIntervalIndex)
    idx.source = idx.data = data
    idx.csr, idx.long, idx.ctx = data.csr(), None, _NoDevice()
    args = (0.8, [1, 0.5], 0.04, 0.25)
    with pytest.raises(ValueError):                                    # min() of an empty cutoff list, cluster.py:188
        idx.score_pairs_any([0], [1], 0.8, [], 0.04, 0.25)
    with pytest.raises(IndexError):
        idx.score_pairs_any([0], [idx.csr.n_reads], *args)
    with pytest.raises(ValueError, match='one length'):
        idx.score_pairs_any([0, 1], [1], *args)
    with pytest.raises(KeyError):
        idx.score_pairs_any(['no such read'], [0], *args)
    ctx = object.__new__(_lib.Context)
    with pytest.raises(ValueError, match='one length'):
        ctx.score_pairs_any([0, 1], [1], 0.96, 0.75, pass_table([1, 0.5]))
    with pytest.raises(ValueError, match='umax'):
        ctx.score_pairs_any([0], [1], 0.96, 0.75, pass_table([1, 0.5]), umax=np.zeros((2, 2), np.int32))


def test_match_python_layer_argument_checks():
    import match_ref as mr
    data = sr.make_data([5, 2, 9, 2], [10, 20, 30, 40], [15, 25, 35, 45])
    idx = object.__new__(cluster.DeviceIntervalIndex)
    idx.source = idx.data = data
    idx.csr, idx.long, idx.ctx = data.csr(), None, _NoDevice()
    new = sr.make_data([2, 9], [12, 31], [22, 33])
    args = (0.8, [1, 0.5], 0.04, 0.25)
    with pytest.raises(ValueError, match='emit'):
        idx.match_reads_any(new, *args, emit='some')
    with pytest.raises(ValueError, match='empty'):
        idx.match_reads_any(new, 0.8, [], 0.04, 0.25)
    with pytest.raises(ValueError, match='exclude'):
        idx.match_reads_any(new, *args, exclude=[0])
    big = mr.resident_data([[(2, 10 * k, 10 * k + 5, 5) for k in range(4097)]], [9], [3])
    with pytest.raises(ValueError, match='query read 0 has more than 4096'):
        idx.match_reads_any(big, *args)
    ctx = object.__new__(_lib.Context)
    with pytest.raises(ValueError, match='umax'):
        ctx.match_reads_any([0, 1], [9], [3], [0], [1], [2], [0], 0.96, 0.75, pass_table([1, 0.5]),
                            umax=np.zeros((2, 2), np.int32))
    with pytest.raises(ValueError, match='read_off'):
        ctx.match_reads_any([], [9], [3], [0], [1], [2], [0], 0.96, 0.75, pass_table([1, 0.5]))


def test_match_reference_on_a_long_resident_read():
    """any_ref.match_ref_any: a long resident read hit by several query intervals is one candidate, at its
    first visit, and agrees with match_ref.match_ref where the pass table reaches."""
    import match_ref as mr
    reads = [ar.diag(70), ar.diag(3), [(1, 5, 900, 895)]]
    data = mr.resident_data(reads, [1000] * 3, [4] * 3)
    csr = data.csr()
    q = mr.Queries([ar.diag(70), [(1, 0, 800_000, 800_000), (1, 10_100, 10_900, 800)], ar.diag(2)], [1000] * 3, [4] * 3)
    off, partner, I, U, flags, counts, best = ar.match_ref_any(data, csr, q, 0.8, ar.CUTS, 0)
    assert counts[:, 0].tolist() == [3, 3, 3] and np.unique(partner[off[1]:off[2]]).size == 3
    long_rank = int(np.argmax(np.diff(csr.read_off)))
    assert (I[0:3].max(), best[0]) == (70, long_rank)
    short = mr.Queries([q.reads[2]], [1000], [4])
    a = ar.match_ref_any(data, csr, short, 0.8, ar.CUTS, 0)
    b = mr.match_ref(data, csr, short, 0.8, ar.QLEN_DIFF, ar.NAL_DIFF, pass_table(ar.CUTS), 0)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def test_multi_gpu_index_raises():
    data = sr.make_data([5, 2], [10, 20], [15, 25])
    with pytest.raises(NotImplementedError, match='multi-GPU'):
        cluster.MultiGpuIndex(data, 2).score_pairs_any([0], [1], 0.8, [1, 0.5], 0.04, 0.25)
    with pytest.raises(NotImplementedError, match='multi-GPU'):
        cluster.MultiGpuIndex(data, 2).match_reads_any(data, 0.8, [1, 0.5], 0.04, 0.25)
