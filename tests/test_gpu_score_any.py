"""Pair scoring for reads of any length on the device (fslr_score_pairs_any / Context.score_pairs_any /
DeviceIntervalIndex.score_pairs_any): lists of 1..4096 intervals against the C oracle's
overall_jaccard_similarity, at the seams of the 64-column chunks and the 64-row slices of the long first-fit,
the width of the result word, the cutoff beyond the pass table, ZeroDivisionError, mixed batches, the
short-only path's equality with fslr_score_pairs, argument errors, state isolation and determinism."""
import ctypes

import numpy as np
import pytest

import any_ref as ar
import long_ref as lr
import search_ref as sr
from any_ref import X, Z, diag, filler, with_at
from fslr_amd import _lib, cluster, synth
from fslr_amd._lib import SCORE_EDGE, SCORE_GATE, SCORE_ZD_GATE, SCORE_ZD_OVERLAP
from fslr_amd.prep import fold_overlap_threshold, pass_table, umax_table

pytestmark = pytest.mark.gpu

QCUT, NCUT = 1 - ar.QLEN_DIFF, 1 - ar.NAL_DIFF


class Loaded:
    """A pool uploaded with fslr_set_reads_any on a context of its own."""

    def __init__(self, pool):
        self.pool, self.ctx = pool, _lib.Context(0)
        csr = pool.csr()
        self.ctx.load_csr_any(csr, fold_overlap_threshold(csr.iv_aln, pool.overlap))

    def score(self, a, b, cuts, umax='auto'):
        if isinstance(umax, str):
            umax = umax_table(cuts, self.pool.max_len())
        return self.ctx.score_pairs_any(a, b, QCUT, NCUT, pass_table(cuts), umax)

    def check(self, a, b, cuts):
        a, b = np.asarray(a, np.int32), np.asarray(b, np.int32)
        I, U, F = self.score(a, b, cuts)
        wI, wU, wF = self.pool.expect(a, b, cuts)
        np.testing.assert_array_equal(I, wI)
        np.testing.assert_array_equal(U, wU)
        np.testing.assert_array_equal(F, wF)
        return I, U, F


def _directed_pool():
    """Every directed read of this module at overlap 0.5, one upload.  Returns (pool, names -> rank)."""
    p, r = ar.Pool(0.5), {}
    for L in ar.SEAM_LENGTHS + (130, 255, 256, 257, 300):
        r['diag', L] = p.add(diag(L))
    r['block_a'] = p.add([X] * 4096)
    r['block_b'] = p.add([X] * 4096)
    # first-fit across chunks: rows 0 and 1 both match columns 0 and 130 alone; row 1 finds column 0 taken
    r['two_rows'] = p.add(with_at(70, 2, {0: X, 1: X}))
    r['cols_0_130'] = p.add(with_at(140, 3, {0: X, 130: X}))
    # a row of list1's third slice that takes column 0
    r['row_130'] = p.add(with_at(140, 2, {130: X}))
    r['col_0'] = p.add(with_at(70, 3, {0: X}))
    # U = 8191: row 0 against column 4095 alone
    r['row0_of_4096'] = p.add(with_at(4096, 2, {0: X}))
    r['col4095_of_4096'] = p.add(with_at(4096, 3, {4095: X}))
    # cutoffs beyond the table
    r['diag65+65'] = p.add(diag(65) + filler(65, 3))            # against diag 65: I = 65, U = 130
    r['diag65+66'] = p.add(diag(65) + filler(66, 3))            # I = 65, U = 131
    r['diag10+119'] = p.add(diag(10) + filler(119, 3))          # against diag(10): I = 10, U = 129
    r['diag10'] = p.add(diag(10))
    r['diag6'] = p.add(diag(6))
    r['diag6+124'] = p.add(diag(6) + filler(124, 3))            # against diag(6): I = 6, U = 130
    r['diag1'] = r['diag', 1]
    # ZeroDivisionError: list1's row 0 is X; list2 holds X at column 130 (chunk 2)
    r['row_x'] = p.add(with_at(70, 2, {0: X}))
    r['zd_ahead'] = p.add(with_at(140, 3, {70: Z, 130: X}))     # the aln_size == 0 column in chunk 1, ahead
    r['zd_behind'] = p.add(with_at(140, 3, {130: X, 135: Z}))   # behind the match
    r['zd_other_chrom'] = p.add(with_at(140, 3, {70: (5, 1000, 2000, 0), 130: X}))
    r['row_z'] = p.add(with_at(70, 2, {0: Z}))                  # an aln_size == 0 row
    r['zd_row_late'] = p.add(with_at(140, 2, {0: X, 135: Z}))   # a zero row of the third slice, after a match
    r['gate_zd_a'] = p.add(diag(130), qlen2=0)
    r['gate_zd_b'] = p.add(diag(129), qlen2=0)
    r['gate_fail'] = p.add(diag(130), qlen2=500, nal=2)
    # the seam gadgets of tests/long_ref.py, swapped and not (first-fit < maximum matching)
    for name, (la, lb, places) in lr.GADGET_PLACES.items():
        for swap in (False, True):
            data = lr.gadgets(la, lb, places, swap)
            rank, lists = lr.rank_of(data), lr.read_lists(data.csr())
            r[name, swap] = (p.add(lists[rank[0]]), p.add(lists[rank[1]]))
    return p, r


@pytest.fixture(scope='module')
def directed():
    pool, names = _directed_pool()
    d = Loaded(pool)
    d.names = names
    yield d
    d.ctx.close()


def test_seams(directed):
    n = directed.names
    pairs = [(n['diag', la], n['diag', lb]) for la in ar.SEAM_LENGTHS for lb in ar.SEAM_LENGTHS]
    pairs += [(n['diag', 129], n['diag', 130]), (n['diag', 130], n['diag', 129]), (n['block_a'], n['block_b'])]
    a, b = zip(*pairs)
    I, U, F = directed.check(a, b, ar.CUTS)
    for k, (la, lb) in enumerate((x, y) for x in ar.SEAM_LENGTHS for y in ar.SEAM_LENGTHS):
        assert (I[k], U[k]) == (min(la, lb), max(la, lb))
    assert (I[-1], U[-1]) == (4096, 4096) and (I[-3], U[-3]) == (129, 130)
    for must in [(1, 65), (65, 1), (64, 65), (65, 64), (65, 65), (4096, 4096)]:
        assert must in [(x, y) for x in ar.SEAM_LENGTHS for y in ar.SEAM_LENGTHS]


def test_first_fit_across_chunks(directed):
    n = directed.names
    pairs = [(n['two_rows'], n['cols_0_130']), (n['row_130'], n['col_0'])]
    for name in lr.GADGET_PLACES:
        for swap in (False, True):
            x, y = n[name, swap]
            pairs += [(x, y), (y, x)]
    a, b = zip(*pairs)
    I, U, F = directed.check(a, b, [0.05])
    assert (I[0], U[0]) == (2, 208) and (I[1], U[1]) == (1, 209)
    # the gadgets are what they claim: first-fit stays below the maximum matching
    pool = directed.pool
    for k in range(2, len(pairs), 2):
        cells = lr.matching_cells(pool.reads[pairs[k][0]], pool.reads[pairs[k][1]], 0.5)
        assert I[k] == lr.first_fit_cells(cells) < lr.max_matching(cells)


def test_result_width(directed):
    n = directed.names
    pairs = [(n['diag', L], n['diag', 300]) for L in (255, 256, 257)]               # I = 255, 256, 257; U = 300
    pairs += [(n['diag', 255], n['diag', 255]), (n['diag', 256], n['diag', 256])]   # U = 255, 256
    pairs += [(n['row0_of_4096'], n['col4095_of_4096']), (n['diag', 300], n['diag', 300])]
    a, b = zip(*pairs)
    I, U, F = directed.check(a, b, [0.0001])
    assert I.tolist() == [255, 256, 257, 255, 256, 1, 300]
    assert U.tolist() == [300, 300, 300, 255, 256, 8191, 300]
    assert (F & SCORE_EDGE).all()


def test_cutoff_beyond_the_table(directed):
    n = directed.names
    a = [n['diag', 65], n['diag', 65], n['diag10'], n['diag6'], n['diag1']]
    b = [n['diag65+65'], n['diag65+66'], n['diag10+119'], n['diag6+124'], n['diag6+124']]
    I, U, F = directed.check(a, b, [0.5])
    assert list(zip(I.tolist(), U.tolist())) == [(65, 130), (65, 131), (10, 129), (6, 130), (1, 130)]
    assert ((F & SCORE_EDGE) != 0).tolist() == [True, False, False, False, False]
    I, U, F = directed.check(a, b, [0.07])                       # 10 / 129 passes: umax decides, not the table
    assert ((F & SCORE_EDGE) != 0).tolist() == [True, True, True, False, False]
    I, U, F = directed.check(a, b, ar.CUTS)                      # I <= 6 with U > 128 under the default cutoffs
    assert ((F & SCORE_EDGE) != 0).tolist() == [True, False, False, False, False]
    directed.check(a, b, [0.001, 0.001, 0.5])                    # I = 1 passes beyond the table, I = 6 does not


def test_zero_division(directed):
    n = directed.names
    a = [n['row_x'], n['row_x'], n['row_x'], n['row_z'], n['zd_row_late'], n['gate_zd_a'], n['gate_fail']]
    b = [n['zd_ahead'], n['zd_behind'], n['zd_other_chrom'], n['cols_0_130'], n['cols_0_130'], n['gate_zd_b'],
         n['diag', 130]]
    I, U, F = directed.check(a, b, ar.CUTS)
    assert F[0] & SCORE_ZD_OVERLAP and (I[0], U[0]) == (0, 0)
    assert not F[1] & SCORE_ZD_OVERLAP and I[1] == 1
    assert not F[2] & SCORE_ZD_OVERLAP and I[2] == 1
    assert F[3] & SCORE_ZD_OVERLAP and F[4] & SCORE_ZD_OVERLAP
    assert F[5] == SCORE_ZD_GATE and (I[5], U[5]) == (129, 130)
    assert F[6] == 0 and (I[6], U[6]) == (130, 130)


def test_mixed_batch_over_several_launches(directed, monkeypatch):
    n = directed.names
    short = [(n['diag10'], n['diag6']), (n['diag', 63], n['diag', 64]), (n['diag6'], n['diag1'])]
    long_ = [(n['diag', 129], n['diag', 65]), (n['two_rows'], n['cols_0_130']), (n['diag', 300], n['diag6']),
             (n['row_x'], n['zd_ahead']), (n['diag', 4096], n['diag', 65])]
    pairs = []
    for k in range(40):                                          # every group of four pairs holds both kinds
        pairs += [short[k % 3], long_[k % 5], short[(k + 1) % 3], long_[(k + 2) % 5]]
    pairs = pairs[:157]                                          # the last wave is partial
    a, b = zip(*pairs)
    want = directed.check(a, b, ar.CUTS)
    monkeypatch.setenv('FSLR_SCORE_CHUNK', '24')                 # seven launches
    got = directed.check(a, b, ar.CUTS)
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()


def test_determinism(directed):
    rng = np.random.default_rng(5)
    n = len(directed.pool.reads)
    keep = [k for k in range(n) if len(directed.pool.reads[k]) <= 300]
    a, b = rng.choice(keep, 400), rng.choice(keep, 400)
    first = directed.score(a, b, ar.CUTS)
    second = directed.score(a, b, ar.CUTS)
    for x, y in zip(first, second):
        assert x.tobytes() == y.tobytes()
    directed.check(a, b, ar.CUTS)


def test_argument_errors(directed):
    ctx, n_real, maxl = directed.ctx, len(directed.pool.reads), directed.pool.max_len()
    assert ctx.n_reads > n_real                                  # virtual chunks follow the real reads
    pt = pass_table(ar.CUTS)
    p = ctx._params(QCUT, NCUT, pt, 0)
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    um = umax_table(ar.CUTS, maxl)

    def call(a, b, umax, n_umax):
        a, b = np.asarray(a, np.int32), np.asarray(b, np.int32)
        I, U, F = np.full(a.size, -7, np.int32), np.full(a.size, -7, np.int32), np.full(a.size, 77, np.uint8)
        rc = ctx._L.fslr_score_pairs_any(ctx._h, ctypes.byref(p), vp(umax) if umax is not None else None, n_umax,
                                         a.size, vp(a), vp(b), vp(I), vp(U), vp(F))
        return rc, ctx._L.fslr_last_error(ctx._h).decode(), (I == -7).all() and (U == -7).all() and (F == 77).all()

    rc, msg, untouched = call([0, 1], [1, 2], None, 0)
    assert rc == _lib.FSLR_ERR_INVALID and 'umax' in msg and untouched
    rc, msg, untouched = call([0, 1], [1, 2], um, maxl - 1)
    assert rc == _lib.FSLR_ERR_INVALID and 'umax' in msg and untouched
    for bad, where in ((n_real, 'a[1]'), (ctx.n_reads - 1, 'b[0]'), (-1, 'b[1]')):
        a, b = [0, 1], [1, 2]
        (a if where[0] == 'a' else b)[int(where[2])] = bad
        rc, msg, untouched = call(a, b, um, maxl)
        assert rc == _lib.FSLR_ERR_INVALID and where in msg and str(bad) in msg and untouched
    rc, msg, untouched = call([0, 1], [1, 2], um, maxl)
    assert rc == _lib.FSLR_OK and not untouched
    assert ctx._L.fslr_score_pairs_any(None, ctypes.byref(p), None, 0, 0, None, None, None, None, None) == \
        _lib.FSLR_ERR_INVALID
    empty = np.zeros(0, np.int32)
    I, U, F = ctx.score_pairs_any(empty, empty, QCUT, NCUT, pt, um)
    assert I.size == U.size == F.size == 0


def test_no_reads_is_a_state_error():
    c = _lib.Context(0)
    try:
        with pytest.raises(_lib.FslrError, match=f'fslr error {_lib.FSLR_ERR_STATE}.*fslr_set_reads'):
            c.score_pairs_any([0], [0], QCUT, NCUT, pass_table(ar.CUTS))
    finally:
        c.close()


def test_short_only_equals_score_pairs():
    s = synth.generate(2000, 16, 23)
    csr = s.interval_data().csr()
    rng = np.random.default_rng(9)
    a, b = rng.integers(0, csr.n_reads, 20_000), rng.integers(0, csr.n_reads, 20_000)
    ctx = _lib.Context(0)
    try:
        ctx.load_csr_any(csr, fold_overlap_threshold(csr.iv_aln, 0.8))       # no long read: plain fslr_set_reads
        assert ctx.n_reads == csr.n_reads
        old = ctx.score_pairs(a, b, QCUT, NCUT, pass_table(ar.CUTS))
        new = ctx.score_pairs_any(a, b, QCUT, NCUT, pass_table(ar.CUTS), None)
        for x, y in zip(old, new):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
        assert (old[2] & SCORE_EDGE).any() and (old[0] > 0).any()
    finally:
        ctx.close()


def _long_index():
    rng = np.random.default_rng(44)
    n = 400
    qcode = np.concatenate([np.zeros(70, np.int64), np.ones(130, np.int64), 2 + rng.integers(0, 60, n - 200)])
    start = rng.integers(0, 200, n) * 500
    data = sr.make_data(rng.integers(1, 3, n), start, start + rng.integers(50, 2500, n), qcode=qcode)
    return data, cluster.build_interval_trees(data)


ARGS = (0.8, ar.CUTS, 0.04, 0.25)


def test_index_method_and_state_isolation():
    data, idx = _long_index()
    ctx = idx.ctx
    try:
        assert idx.long is not None and int(idx.long.max()) == 130
        csr = idx.csr
        n = csr.n_reads
        thr = fold_overlap_threshold(csr.iv_aln, 0.8)
        ctx.set_thresholds(thr)
        ctx.set_long_cutoffs(umax_table(ar.CUTS, 130))
        ctx.reserve_edges(1 << 16)
        n_long = ctx.long_query(QCUT, NCUT, pass_table(ar.CUTS))
        ne = ctx.stats()['n_edges']
        ctx.components()
        labels, edges, long_edges = ctx.labels(), ctx.edges(ne), ctx.long_edges(n_long)
        dense = idx._dense_chroms(data.chrom[:100])
        qs, qe = idx._coords(data.start[:100]), idx._coords(data.end[:100])
        want_off, want_hits = ctx.search(dense, qs, qe)
        total = ctx._search(dense, qs, qe, None)                 # a saved search batch, its hits not yet fetched
        # every ordered pair of real reads through the index method, against the oracle over whole lists
        a, b = (x.ravel() for x in np.meshgrid(np.arange(n), np.arange(n), indexing='ij'))
        r = idx.score_pairs_any(a, b, *ARGS)
        lists = lr.read_lists(csr)
        pool = ar.Pool(0.8)
        for k in range(n):
            pool.add(lists[k], int(csr.read_qlen2[k]), int(csr.read_nal[k]))
        wI, wU, wF = pool.expect(a, b, ar.CUTS)
        np.testing.assert_array_equal(r.I, wI)
        np.testing.assert_array_equal(r.U, wU)
        np.testing.assert_array_equal(r.flags, wF)
        assert r.I.max() > 64 and len(r) == n * n
        # the query state and the saved search batch are as they were
        np.testing.assert_array_equal(ctx.labels(), labels)
        for x, y in zip(ctx.edges(ne), edges):
            np.testing.assert_array_equal(x, y)
        for x, y in zip(ctx.long_edges(n_long), long_edges):
            np.testing.assert_array_equal(x, y)
        hits = np.full(total, -7, np.int32)
        ctx._check(ctx._L.fslr_search_hits(ctx._h, hits.ctypes.data_as(ctypes.c_void_p), total))
        np.testing.assert_array_equal(hits, want_hits)
        # the old method keeps refusing
        with pytest.raises(NotImplementedError, match='64'):
            idx.score_pairs([0], [1], *ARGS)
    finally:
        ctx.close()
    with pytest.raises(NotImplementedError, match='multi-GPU'):
        cluster.MultiGpuIndex(data, 2).score_pairs_any([0], [1], *ARGS)
