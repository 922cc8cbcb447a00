"""The first-fit matching of scored pairs on the device (fslr_pair_matching / fslr_pair_matching_any /
Context.pair_matching / DeviceIntervalIndex.score_pairs(matching=True)): per pair, which interval of list1 took
which interval of list2, against the plain statement of tests/matching_ref.py and the fixture recorded from the
reference; I, U and flags against the oracle and against fslr_score_pairs on the same batch."""
import ctypes
import os

import numpy as np
import pytest

import any_ref as ar
import fixtures as fx
import host_pipeline as hp
import matching_ref as mr
from any_ref import X, Z, diag, filler, with_at
from fslr_amd import _lib, cluster, synth
from fslr_amd._lib import SCORE_EDGE, SCORE_ZD_GATE, SCORE_ZD_OVERLAP
from fslr_amd.prep import fold_overlap_threshold, pass_table, umax_table

pytestmark = pytest.mark.gpu

QCUT, NCUT = 1 - ar.QLEN_DIFF, 1 - ar.NAL_DIFF
PT = pass_table(ar.CUTS)
FAR = (1, 500_000, 501_000, 1000)             # matches nothing a test builds


class Loaded:
    """A pool on a context of its own: fslr_set_reads_any where it holds a read of more than 64 intervals."""

    def __init__(self, pool, ctx=None):
        self.pool, self.ctx = pool, ctx or _lib.Context(0)
        self.virt = pool.max_len() > _lib.FSLR_MAX_L
        csr = pool.csr()
        (self.ctx.load_csr_any if self.virt else self.ctx.load_csr)(csr, fold_overlap_threshold(csr.iv_aln, pool.overlap))

    def call(self, a, b, plain=None):
        plain = not self.virt if plain is None else plain
        if plain:
            return self.ctx.pair_matching(a, b, QCUT, NCUT, PT)
        return self.ctx.pair_matching_any(a, b, QCUT, NCUT, PT, umax_table(ar.CUTS, self.pool.max_len()))

    def score(self, a, b):
        if not self.virt:
            return self.ctx.score_pairs(a, b, QCUT, NCUT, PT)
        return self.ctx.score_pairs_any(a, b, QCUT, NCUT, PT, umax_table(ar.CUTS, self.pool.max_len()))

    def check(self, a, b, plain=None):
        """One call against the references; returns its six arrays."""
        a, b = np.asarray(a, np.int32), np.asarray(b, np.int32)
        got = self.call(a, b, plain)
        I, U, F, off, i, j = got
        for g, w in zip((I, U, F), self.pool.expect(a, b, ar.CUTS)):
            np.testing.assert_array_equal(g, w)
        for g, w in zip((I, U, F), self.score(a, b)):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
        mr.check((off, i, j), mr.expect(self.pool.reads, a, b, self.pool.overlap), I, F)
        return got


def same_bytes(x, y):
    for g, w in zip(x, y):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()


# ------------------------------------------------------------------ 1. KATs and the golden fixture
def test_kat_jaccard():
    kats = fx.kats()['jaccard']
    c = _lib.Context(0)
    try:
        rows = raised = 0
        for pct in sorted({k['pct'] for k in kats}):
            pool = ar.Pool(pct)
            for t, k in enumerate(kats):
                if k['pct'] == pct and k['a'] and k['b']:
                    base = 10_000 + (t % 1000) * 10_000
                    for lst in (k['a'], k['b']):
                        pool.add([(ch, s + base, e + base, al) for ch, s, e, al in lst])
            n = len(pool.reads) // 2
            ts = np.arange(n)
            I, U, F, off, i, j = Loaded(pool, c).check(np.concatenate([2 * ts, 2 * ts + 1]),
                                                       np.concatenate([2 * ts + 1, 2 * ts]))
            rows += i.size
            raised += int(((F & SCORE_ZD_OVERLAP) != 0).sum())
        assert rows > 1000 and raised >= 1
    finally:
        c.close()


def test_golden_fixture():
    """What the reference itself did (tests/golden/matching/pairs.npz), through the index method."""
    z = np.load(os.path.join(fx.GOLDEN, 'matching', 'pairs.npz'))
    c = _lib.Context(0)
    try:
        for name in z['sources'].tolist():
            data, _, _ = hp.host_prepare(name)
            idx = cluster.build_interval_trees(data, ctx=c)
            a, b = z[f'{name}_a'], z[f'{name}_b']
            r = idx.score_pairs(a, b, float(z[f'{name}_pct']), ar.CUTS, ar.QLEN_DIFF, ar.NAL_DIFF, matching=True)
            m = r.matching
            np.testing.assert_array_equal(m.offsets, z[f'{name}_off'])
            np.testing.assert_array_equal(m.i, z[f'{name}_i'])
            np.testing.assert_array_equal(m.j, z[f'{name}_j'])
            np.testing.assert_array_equal((r.flags & SCORE_ZD_OVERLAP) != 0, z[f'{name}_raised'])
            np.testing.assert_array_equal(r.I, np.diff(m.offsets))
            s = idx.score_pairs(a, b, float(z[f'{name}_pct']), ar.CUTS, ar.QLEN_DIFF, ar.NAL_DIFF)
            same_bytes((r.I, r.U, r.flags), (s.I, s.U, s.flags))
    finally:
        c.close()


# ------------------------------------------------------------------ 2. lane groups
LB = (1, 15, 16, 17, 31, 32, 33, 63, 64)
LA = (1, 16, 17, 33, 64)


def lane_pool():
    """Dense reads on two chromosomes (a row has several candidate columns), one per length of LA and LB."""
    rng = np.random.default_rng(8)
    pool, rank = ar.Pool(0.8), {}
    for side, lengths in (('a', LA), ('b', LB)):
        for L in lengths:
            s, w = rng.integers(0, 200, L), rng.integers(85, 115, L)
            rank[side, L] = pool.add([(int(c), int(x), int(x + y), int(y)) for c, x, y in zip(rng.integers(0, 2, L), s, w)],
                                     int(rng.integers(900, 1100)), int(rng.integers(3, 6)))
    return pool, rank


@pytest.fixture(scope='module')
def lanes():
    pool, rank = lane_pool()
    d = Loaded(pool)
    d.rank = rank
    yield d
    d.ctx.close()


def test_lane_groups(lanes):
    r = lanes.rank
    pairs = [(r['a', la], r['b', lb]) for la in LA for lb in LB]
    # single waves of four with mixed widths: a 16-lane pair riding in a 32- and in a 64-lane wave
    mixed = [(r['a', 17], r['b', 15]), (r['a', 1], r['b', 33]), (r['a', 64], r['b', 1]), (r['a', 16], r['b', 64]),
             (r['a', 33], r['b', 16]), (r['a', 17], r['b', 17]), (r['a', 1], r['b', 1]), (r['a', 64], r['b', 31]),
             (r['a', 16], r['b', 16]), (r['a', 16], r['b', 15]), (r['a', 64], r['b', 1]), (r['a', 33], r['b', 15])]
    a, b = (np.array(x) for x in zip(*(pairs + mixed)))
    I, U, F, off, i, j = lanes.check(a, b)
    assert I.max() >= 16 and (I == 0).sum() < I.size // 2
    for n in (1, 3, 4, 5):                                      # the tail wave
        for k0 in (0, len(pairs), len(pairs) + 4):
            lanes.check(a[k0:k0 + n], b[k0:k0 + n])
    # a pair's rows do not depend on its neighbours in the wave
    for k in range(len(pairs), a.size):
        one = lanes.call(a[k:k + 1], b[k:k + 1])
        assert one[4].tolist() == i[off[k]:off[k + 1]].tolist() and one[5].tolist() == j[off[k]:off[k + 1]].tolist()


# ------------------------------------------------------------------ 3. the shape of the matching, 4. ZeroDivisionError
OTHER = (2, 1000, 2000, 1000)


def shape_pool():
    p, r = ar.Pool(0.8), {}
    r['x_other'] = p.add([X, OTHER])
    r['other_far_x'] = p.add([OTHER, FAR, X])                   # row 0 takes column 2, row 1 column 0
    r['x_far_x_x'] = p.add([X, FAR, X, X])
    r['xx'] = p.add([X, X])                                     # unmatched rows between and behind matched ones
    r['xxx'] = p.add([X, X, X])
    r['x'] = p.add([X])                                         # a taken column that later rows would also match
    r['chroms_a'] = p.add([(c, 1000, 2000, 1000) for c in (3, 1, 2, 3, 1)])
    r['chroms_b'] = p.add([(c, 1000, 2000, 1000) for c in (1, 3, 3, 2, 4)])
    r['diag9'] = p.add(diag(9))
    r['diag9+'] = p.add(diag(9) + filler(5, 3))                 # I = min(LA, LB)
    r['far'] = p.add([FAR, FAR])                                # I = 0 against everything above
    # ZeroDivisionError
    r['z_x'] = p.add([Z, X])                                    # raises at row 0
    r['xxz'] = p.add([X, X, Z])                                 # list1 = xxx: raises after two matches
    r['gate_zd'] = p.add([X, X], qlen2=0)                       # the gate raises, the overlap does not
    r['gate_zd2'] = p.add([X, FAR, X], qlen2=0)
    return p, r


@pytest.fixture(scope='module')
def shapes():
    pool, rank = shape_pool()
    d = Loaded(pool)
    d.rank = rank
    yield d
    d.ctx.close()


def rows_of(got, k):
    I, U, F, off, i, j = got
    return list(zip(i[off[k]:off[k + 1]].tolist(), j[off[k]:off[k + 1]].tolist()))


def test_shape_of_the_matching(shapes):
    r = shapes.rank
    pairs = [('x_other', 'other_far_x'), ('far', 'xx'), ('x_far_x_x', 'xx'), ('xxx', 'x'), ('far', 'far'),
             ('chroms_a', 'chroms_b'), ('xx', 'far'), ('diag9', 'diag9+'), ('diag9+', 'diag9'), ('far', 'x'), ('x', 'x')]
    got = shapes.check([r[x] for x, _ in pairs], [r[y] for _, y in pairs])
    assert rows_of(got, 0) == [(0, 2), (1, 0)]
    assert rows_of(got, 2) == [(0, 0), (2, 1)]
    assert rows_of(got, 3) == [(0, 0)]
    assert rows_of(got, 4) == [(0, 0), (1, 1)]                  # a == b is a pair like any other
    assert rows_of(got, 5) == [(0, 1), (1, 0), (2, 3), (3, 2)]
    assert rows_of(got, 7) == rows_of(got, 8) == [(k, k) for k in range(9)]
    assert [rows_of(got, k) for k in (1, 6, 9)] == [[], [], []] and rows_of(got, 10) == [(0, 0)]


def test_zero_division(shapes):
    r = shapes.rank
    pairs = [('x', 'z_x'), ('x_other', 'other_far_x'), ('xxx', 'xxz'), ('xx', 'xxx'), ('gate_zd', 'gate_zd2'),
             ('gate_zd2', 'gate_zd'), ('z_x', 'x'), ('xxx', 'x')]
    got = shapes.check([r[x] for x, _ in pairs], [r[y] for _, y in pairs])
    I, U, F, off, i, j = got
    for k in (0, 2, 6):                                         # at row 0; after two matches; a zero row
        assert F[k] & SCORE_ZD_OVERLAP and (I[k], U[k]) == (0, 0) and rows_of(got, k) == []
    assert rows_of(got, 1) == [(0, 2), (1, 0)] and rows_of(got, 3) == [(0, 0), (1, 1)] and rows_of(got, 7) == [(0, 0)]
    # a gate ZeroDivisionError still has its rows
    assert F[4] & SCORE_ZD_GATE and not F[4] & SCORE_ZD_OVERLAP and rows_of(got, 4) == [(0, 0), (1, 2)]
    assert F[5] & SCORE_ZD_GATE and rows_of(got, 5) == [(0, 0), (2, 1)]


# ------------------------------------------------------------------ 5. chunk seams
def test_chunk_seams(lanes, monkeypatch):
    rng = np.random.default_rng(5)
    n = len(lanes.pool.reads)
    a, b = rng.integers(0, n, 37), rng.integers(0, n, 37)
    want = lanes.check(a, b)
    assert want[3][-1] > 100
    for env in ({'FSLR_SCORE_CHUNK': '8'}, {'FSLR_SCORE_CHUNK': '1'}, {'FSLR_MATCHING_ROWS': '64'},
                {'FSLR_SCORE_CHUNK': '8', 'FSLR_MATCHING_ROWS': '1'}):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            same_bytes(lanes.check(a, b), want)
    with monkeypatch.context() as m:
        m.setenv('FSLR_SCORE_CHUNK', '0')
        with pytest.raises(_lib.FslrError, match='FSLR_SCORE_CHUNK'):
            lanes.call(a, b)


# ------------------------------------------------------------------ 6. any length
def long_pool():
    p, r = ar.Pool(0.5), {}
    for L in (1, 3, 64, 65, 128, 129, 4096):
        r['diag', L] = p.add(diag(L))
    r['diag4096b'] = p.add(diag(4096))
    r['x'] = p.add([X])
    r['x_at_4000_of_4096'] = p.add(with_at(4096, 2, {4000: X}))
    # the chunk-outer seam: row 0's only match is column 70, row 1's is column 3
    Y = (1, 30_000, 31_000, 1000)
    r['rows_x_y'] = p.add(with_at(70, 2, {0: X, 1: Y}))
    r['cols_y3_x70'] = p.add(with_at(140, 3, {3: Y, 70: X}))
    # a row left pending through two full chunks: row 0 matches column 130 alone, rows 1 and 2 columns 0 and 64
    W = (1, 60_000, 61_000, 1000)
    r['rows_x_y_w'] = p.add(with_at(70, 2, {0: X, 1: Y, 2: W}))
    r['cols_y0_w64_x130'] = p.add(with_at(140, 3, {0: Y, 64: W, 130: X}))
    # a chunk whose columns are all taken before the last slice: 64 columns that rows 0..63 take, the rows of
    # the second and third slices find chunk 0 full and go on to chunk 1
    r['rows_130x'] = p.add([X] * 130)
    r['cols_100x'] = p.add([X] * 100)
    # a raise in the second chunk: row 0 matches nothing in chunk 0 and meets the aln_size == 0 column 70
    r['row_x'] = p.add(with_at(70, 2, {0: X}))
    r['zd_70_x_130'] = p.add(with_at(140, 3, {70: Z, 130: X}))
    r['short_a'] = p.add([X, FAR, X])
    r['short_b'] = p.add([FAR, X, X, X])
    r['short_c'] = p.add(diag(17))
    return p, r


@pytest.fixture(scope='module')
def longs():
    pool, rank = long_pool()
    d = Loaded(pool)
    d.rank = rank
    yield d
    d.ctx.close()


def test_any_length_seams(longs):
    r = longs.rank
    assert longs.virt and longs.ctx.n_reads > len(longs.pool.reads)
    pairs = [(r['diag', la], r['diag', lb]) for la, lb in ((65, 3), (3, 65), (64, 65), (128, 129), (129, 128))]
    pairs += [(r['diag', 4096], r['x']), (r['x_at_4000_of_4096'], r['x']), (r['x'], r['x_at_4000_of_4096'])]
    got = longs.check(*zip(*pairs))
    for k, n in enumerate((3, 3, 64, 128, 128)):
        assert rows_of(got, k) == [(x, x) for x in range(n)]
    assert rows_of(got, 5) == [] and rows_of(got, 6) == [(4000, 0)] and rows_of(got, 7) == [(0, 4000)]


def test_any_length_diagonal_4096(longs):
    r = longs.rank
    I, U, F, off, i, j = longs.call([r['diag', 4096]], [r['diag4096b']])
    assert (I[0], U[0]) == (4096, 4096) and off.tolist() == [0, 4096]
    np.testing.assert_array_equal(i, np.arange(4096))
    np.testing.assert_array_equal(j, np.arange(4096))
    same_bytes((I, U, F), longs.score([r['diag', 4096]], [r['diag4096b']]))


def test_any_length_chunk_outer(longs):
    r = longs.rank
    pairs = [('rows_x_y', 'cols_y3_x70'), ('rows_x_y_w', 'cols_y0_w64_x130'), ('rows_130x', 'cols_100x'),
             ('row_x', 'zd_70_x_130'), ('cols_100x', 'rows_130x'), ('rows_x_y', 'cols_y3_x70')]
    got = longs.check([r[x] for x, _ in pairs], [r[y] for _, y in pairs])
    assert rows_of(got, 0) == rows_of(got, 5) == [(0, 70), (1, 3)]              # rows 0 then 1, not chunk order
    assert rows_of(got, 1) == [(0, 130), (1, 0), (2, 64)]
    assert rows_of(got, 2) == [(k, k) for k in range(100)] == rows_of(got, 4)
    assert got[2][3] & SCORE_ZD_OVERLAP and rows_of(got, 3) == []


def test_long_pair_beside_short_ones(longs):
    r = longs.rank
    short = [(r['short_a'], r['short_b']), (r['short_c'], r['short_c']), (r['short_b'], r['short_a'])]
    lng = (r['rows_x_y_w'], r['cols_y0_w64_x130'])
    want = {p: rows_of(longs.check([p[0]], [p[1]]), 0) for p in short + [lng]}
    for batch in ([lng] + short, short + [lng], short[:2] + [lng] + short[2:] + short + [lng, lng]):
        got = longs.check(*zip(*batch))
        assert [rows_of(got, k) for k in range(len(batch))] == [want[p] for p in batch]


def test_any_equals_plain_without_long_reads(lanes):
    rng = np.random.default_rng(6)
    n = len(lanes.pool.reads)
    a, b = rng.integers(0, n, 203), rng.integers(0, n, 203)
    same_bytes(lanes.check(a, b, plain=True), lanes.check(a, b, plain=False))
    same_bytes(lanes.ctx.pair_matching_any(a, b, QCUT, NCUT, PT, None), lanes.check(a, b, plain=True))


# ------------------------------------------------------------------ 7. consistency at size
def test_consistent_at_size():
    csr = synth.generate(20_000, 16, 31).interval_data().csr()
    n = csr.n_reads
    thr = fold_overlap_threshold(csr.iv_aln, 0.8)
    c = _lib.Context(0)
    try:
        c.load_csr(csr, thr)
        c.reserve_edges(max(1 << 16, 12 * n))
        c.build_index()
        st = c.run_query(QCUT, NCUT, PT, edge_threshold=1 << 30)
        ea, eb, _, _ = c.edges(st['n_edges'])
        order = np.lexsort((eb, ea))                             # (the edges lie in HBM in no fixed order)
        ea, eb = ea[order], eb[order]
        rng = np.random.default_rng(3)
        keep = rng.permutation(ea.size)[:10_000]
        ra = rng.integers(0, n, keep.size)
        a = np.concatenate([ea[keep], ra]).astype(np.int32)
        b = np.concatenate([eb[keep], np.minimum(ra + rng.integers(0, 3, keep.size), n - 1)]).astype(np.int32)
        assert 2000 <= a.size <= 20_000
        first = c.pair_matching(a, b, QCUT, NCUT, PT)
        I, U, F, off, i, j = first
        same_bytes((I, U, F), c.score_pairs(a, b, QCUT, NCUT, PT))
        k = np.repeat(np.arange(a.size), np.diff(off))
        assert off[-1] == i.size == j.size == I.sum() > 10_000 and (np.diff(off) == I).all()
        ro = np.asarray(csr.read_off, np.int64)
        p1, p2 = ro[a[k]] + i, ro[b[k]] + j
        assert (i >= 0).all() and (p1 < ro[a[k] + 1]).all() and (j >= 0).all() and (p2 < ro[b[k] + 1]).all()
        # every row is a real match: the chromosomes are equal and the shared span reaches both thresholds
        shared = np.minimum(csr.iv_end[p1], csr.iv_end[p2]).astype(np.int64) - np.maximum(csr.iv_start[p1], csr.iv_start[p2])
        assert (csr.iv_chrom[p1] == csr.iv_chrom[p2]).all()
        assert (shared / csr.iv_aln[p1] >= 0.8).all() and (shared / csr.iv_aln[p2] >= 0.8).all()
        inner = k[1:] == k[:-1]
        assert (i[1:][inner] > i[:-1][inner]).all()                           # rows strictly ascending per pair
        assert np.unique(k * 64 + j).size == j.size                           # columns distinct per pair
        dp = np.asarray(csr.data_pos, np.int64)
        reads = [list(zip(csr.iv_chrom[s:e].tolist(), csr.iv_start[s:e].tolist(), csr.iv_end[s:e].tolist(),
                          csr.iv_aln[s:e].tolist())) for s, e in zip(ro[:-1].tolist(), ro[1:].tolist())]
        assert dp.size == ro[-1]
        mr.check((off, i, j), mr.expect(reads, a, b, 0.8), I, F)
        same_bytes(c.pair_matching(a, b, QCUT, NCUT, PT), first)
    finally:
        c.close()


# ------------------------------------------------------------------ 8. errors and state
def raw_call(ctx, a, b, capacity, rows=True, n_pairs=None, any_umax=None):
    """The C call with sentinel-filled outputs: (rc, message, outputs dict)."""
    a, b = np.asarray(a, np.int32), np.asarray(b, np.int32)
    n = a.size if n_pairs is None else n_pairs
    o = dict(I=np.full(a.size, -7, np.int32), U=np.full(a.size, -7, np.int32), F=np.full(a.size, 77, np.uint8),
             off=np.full(a.size + 1, -7, np.int64), row=np.full(max(capacity, 1), -7, np.int32),
             col=np.full(max(capacity, 1), -7, np.int32))
    total = ctypes.c_int64(-7)
    p = ctx._params(QCUT, NCUT, PT, 0)
    vp = _lib._ptr
    tail = (n, vp(a), vp(b), vp(o['I']), vp(o['U']), vp(o['F']), vp(o['off']), vp(o['row']) if rows else None,
            vp(o['col']) if rows else None, capacity, ctypes.byref(total))
    if any_umax is not None:
        rc = ctx._L.fslr_pair_matching_any(ctx._h, ctypes.byref(p), vp(any_umax), any_umax.size, *tail)
    else:
        rc = ctx._L.fslr_pair_matching(ctx._h, ctypes.byref(p), *tail)
    o['n_rows'] = total.value
    return rc, ctx._L.fslr_last_error(ctx._h).decode(), o


def untouched(o):
    return ((o['I'] == -7).all() and (o['U'] == -7).all() and (o['F'] == 77).all() and (o['off'] == -7).all()
            and (o['row'] == -7).all() and (o['col'] == -7).all() and o['n_rows'] == -7)


def test_errors_and_capacity(lanes, longs):
    ctx = lanes.ctx
    n = len(lanes.pool.reads)
    for bad, where in ((-1, 'a[0]'), (n, 'b[3]')):
        a, b = [0, 1, 2, 3], [1, 2, 3, 4]
        (a if where[0] == 'a' else b)[int(where[2])] = bad
        rc, msg, o = raw_call(ctx, a, b, 256)
        assert rc == _lib.FSLR_ERR_INVALID and where in msg and str(bad) in msg and untouched(o)
    a, b = np.arange(n - 1), np.arange(1, n)
    I, U, F, off, i, j = lanes.check(a, b)
    total = int(off[-1])
    assert total > 10
    rc, msg, o = raw_call(ctx, a, b, total)
    assert rc == _lib.FSLR_OK and o['n_rows'] == total
    np.testing.assert_array_equal(o['row'][:total], i)
    np.testing.assert_array_equal(o['col'][:total], j)
    rc, msg, o = raw_call(ctx, a, b, total - 1)                  # one short
    assert rc == _lib.FSLR_ERR_INVALID and str(total) in msg and o['n_rows'] == total
    for g, w in ((o['I'], I), (o['U'], U), (o['F'], F), (o['off'], off)):
        np.testing.assert_array_equal(g, w)
    rc, msg, o = raw_call(ctx, a, b, 0, rows=False)              # count only
    assert rc == _lib.FSLR_OK and o['n_rows'] == total
    np.testing.assert_array_equal(o['off'], off)
    np.testing.assert_array_equal(o['I'], I)
    rc, msg, o = raw_call(ctx, a[:0], b[:0], 0, rows=False)      # n_pairs == 0
    assert rc == _lib.FSLR_OK and o['n_rows'] == 0 and o['off'].tolist() == [0]
    e = lanes.call(a[:0], b[:0])
    assert [x.size for x in e] == [0, 0, 0, 1, 0, 0]
    # virtual reads: the plain call refuses, the _any call wants umax and real ranks
    lctx, n_real = longs.ctx, len(longs.pool.reads)
    rc, msg, o = raw_call(lctx, [0], [1], 16)
    assert rc == _lib.FSLR_ERR_INVALID and '64' in msg and untouched(o)
    um = umax_table(ar.CUTS, longs.pool.max_len()).astype(np.int32)
    rc, msg, o = raw_call(lctx, [0], [1], 16, any_umax=um[:100])
    assert rc == _lib.FSLR_ERR_INVALID and 'umax' in msg and untouched(o)
    rc, msg, o = raw_call(lctx, [0, n_real], [1, 0], 16, any_umax=um)
    assert rc == _lib.FSLR_ERR_INVALID and 'a[1]' in msg and untouched(o)


def test_no_reads_is_a_state_error():
    c = _lib.Context(0)
    try:
        with pytest.raises(_lib.FslrError, match=f'fslr error {_lib.FSLR_ERR_STATE}.*fslr_set_reads'):
            c.pair_matching([0], [0], QCUT, NCUT, PT)
        with pytest.raises(_lib.FslrError, match=f'fslr error {_lib.FSLR_ERR_STATE}.*fslr_set_reads'):
            c.pair_matching_any([0], [0], QCUT, NCUT, PT)
    finally:
        c.close()


def test_other_state_is_left_alone():
    csr = synth.generate(2000, 16, 11).interval_data().csr()
    thr = fold_overlap_threshold(csr.iv_aln, 0.8)
    c = _lib.Context(0)
    try:
        c.load_csr(csr, thr)
        c.reserve_edges(1 << 16)
        c.build_index()
        st = c.run_query(QCUT, NCUT, PT)
        c.components()

        def state():
            return (*c.edges(st['n_edges']), c.labels(), c.fwd_degree())
        before = state()
        qs = (csr.iv_chrom[:300], csr.iv_start[:300], csr.iv_end[:300])
        want_off, want_hits = c.search(*qs)
        match_args = (csr.read_off, csr.read_qlen2, csr.read_nal, csr.iv_chrom, csr.iv_start, csr.iv_end, thr, QCUT,
                      NCUT, PT, SCORE_EDGE, np.arange(csr.n_reads))
        c.match_reads(*match_args)
        want_rows = c.match_rows()
        total = c._search(*qs, None)                              # a saved search batch
        c.match_reads(*match_args)                                # a saved match batch
        got = c.pair_matching(np.arange(500), np.arange(1, 501), QCUT, NCUT, PT)
        assert got[3][-1] == got[0].sum()
        hits = np.full(total, -7, np.int32)
        c._check(c._L.fslr_search_hits(c._h, _lib._ptr(hits), total))
        np.testing.assert_array_equal(hits, want_hits)
        same_bytes(c.match_rows(), want_rows)
        for x, y in zip(before, state()):
            np.testing.assert_array_equal(x, y)
    finally:
        c.close()


# ------------------------------------------------------------------ 9. Python
def test_index_method():
    data, _, _ = hp.host_prepare('ties_600')
    idx = cluster.build_interval_trees(data)
    try:
        n = idx.csr.n_reads
        args = (0.8, ar.CUTS, ar.QLEN_DIFF, ar.NAL_DIFF)
        a, b = np.arange(n - 1), np.arange(1, n)
        names = idx.data.qnames[idx.csr.read_qcode]
        r = idx.score_pairs(a, b, *args, matching=True)
        q = idx.score_pairs(list(names[a]), list(names[b]), *args, matching=True)
        plain = idx.score_pairs(a, b, *args)
        assert plain.matching is None and idx.score_pairs(a, b, *args, matching=False).matching is None
        assert list(plain.to_frame().columns) == ['query1', 'query2', 'jaccard_similarity', 'n_i', 'gate', 'edge']
        for f in ('a', 'b', 'I', 'U', 'flags', 'jaccard', 'gate', 'edge', 'zero_division'):
            np.testing.assert_array_equal(getattr(r, f), getattr(plain, f))
            np.testing.assert_array_equal(getattr(q, f), getattr(plain, f))
        m = r.matching
        for f in ('offsets', 'i', 'j'):
            np.testing.assert_array_equal(getattr(m, f), getattr(q.matching, f))
        assert len(m) == r.I.sum() > 100
        ma = idx.score_pairs_any(a, b, *args, matching=True).matching
        same_bytes((m.offsets, m.i, m.j), (ma.offsets, ma.i, ma.j))
        f = m.to_frame()
        assert list(f.columns) == ['query1', 'query2', 'i', 'j', 'chrom1', 'start1', 'end1', 'chrom2', 'start2', 'end2']
        assert f.equals(q.matching.to_frame()) and len(f) == len(m)
        k = m.pair_of_row()
        assert f['query1'].tolist() == list(names[a[k]]) and f['query2'].tolist() == list(names[b[k]])
        # the frame's intervals are the reads' own: interval i of query1 in the `data` list
        lists = {}
        for pos in range(len(data)):
            lists.setdefault(data.qnames[data.qcode[pos]], []).append(pos)
        for row in f.iloc[::7].itertuples():
            p1, p2 = lists[row.query1][row.i], lists[row.query2][row.j]
            assert (row.chrom1, row.start1, row.end1) == (data.chrom[p1], data.start[p1], data.end[p1])
            assert (row.chrom2, row.start2, row.end2) == (data.chrom[p2], data.start[p2], data.end[p2])
            assert row.chrom1 == row.chrom2
        assert idx.score_pairs([], [], *args, matching=True).matching.to_frame().shape == (0, 10)
    finally:
        idx.ctx.close()
    with pytest.raises(NotImplementedError, match='multi-GPU'):
        cluster.MultiGpuIndex(data, 2).score_pairs([0], [1], 0.8, ar.CUTS, ar.QLEN_DIFF, ar.NAL_DIFF, matching=True)
