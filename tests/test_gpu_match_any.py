"""Matching new reads of any length against a resident index that may hold reads of more than 64 intervals
(fslr_match_reads_any / fslr_match_rows_any / DeviceIntervalIndex.match_reads_any): rows, their order, counts
and best against tests/any_ref.match_ref_any (brute-force search reduced to first visits of real reads, the C
oracle over whole lists, the float cutoff rule).  Every query read of every input is compared."""
import numpy as np
import pytest

import any_ref as ar
import match_ref as mr
from fslr_amd import _lib, cluster, synth
from fslr_amd._lib import MATCH_SET, SCORE_EDGE, SCORE_GATE, SCORE_ZD_OVERLAP
from fslr_amd.prep import fold_overlap_threshold, pass_table, umax_table

pytestmark = pytest.mark.gpu

PCT = 0.8
NAMES = ('offsets', 'partner', 'I', 'U', 'flags', 'counts', 'best')
N_SINGLE = 300


def same(got, want, what=''):
    for name, g, w in zip(NAMES, got, want):
        np.testing.assert_array_equal(g, w, err_msg=f'{what} {name}')


def run_any(ctx, data, q, cuts, emit_mask, max_len, exclude='own', umax='auto'):
    ex = q.exclude if isinstance(exclude, str) else exclude
    if isinstance(umax, str):
        umax = umax_table(cuts, max(max_len, int(np.diff(q.off).max(initial=1))))
    off, counts, best = ctx.match_reads_any(q.off, q.qlen2, q.nal, q.dense_chrom(data), q.flat[:, 1], q.flat[:, 2],
                                            fold_overlap_threshold(q.flat[:, 3], PCT), 1 - ar.QLEN_DIFF,
                                            1 - ar.NAL_DIFF, pass_table(cuts), emit_mask, ex, umax=umax)
    return (off, *ctx.match_rows_any(), counts, best)


def long_read(n, shift):
    return [(1, 10_000 * k + shift, 10_000 * k + shift + 1000, 1000) for k in range(n)]


def single(j):
    return (2, 5000 * j, 5000 * j + 1000, 1000)


def resident():
    """383 reads: three long ones (65, 130 and 4096 intervals, interleaved on chromosome 1), 80 random short
    reads over the first 130 of their places (some with an aln_size == 0 interval, some failing the length
    gate) and 300 one-interval reads on chromosome 2."""
    rng = np.random.default_rng(3)
    reads = [long_read(65, 0), long_read(130, 300), long_read(4096, 600)]
    qlen2, nal = [1000, 1000, 1000], [4, 4, 4]
    for t in range(80):
        L = int(rng.integers(1, 17))
        ks = np.sort(rng.choice(130, L, replace=False))
        r = [(1, 10_000 * int(k) + int(rng.integers(0, 700)), 0, 1000) for k in ks]
        r = [(c, s, s + 1000, 0 if t % 9 == 4 and i == 0 else a) for i, (c, s, _, a) in enumerate(r)]
        reads.append(r)
        qlen2.append(500 if t % 5 == 0 else 1000)
        nal.append(2 if t % 5 == 0 else 4)
    for j in range(N_SINGLE):
        reads.append([single(j)])
        qlen2.append(1000)
        nal.append(4)
    return mr.resident_data(reads, qlen2, nal), reads


def queries(reads):
    jit = lambda r, d: [(c, s + d, e + d, a) for c, s, e, a in r]
    q = [
        # one interval over four chunks of the 4096-read and both chunks of the others, then short ones on them
        [(1, 0, 2_000_000, 2_000_000), (1, 700_100, 701_000, 900), (1, 1_280_400, 1_281_300, 900), (1, 100, 900, 800)],
        jit(reads[0][:64], 5),                      # 64 intervals
        jit(reads[0], 5),                           # 65
        jit(reads[1][:129], -5),                    # 129
        jit(reads[2], 7),                           # 4096
        jit(reads[10], 3),                          # a short read against short and long partners
        # more than FSLR_MATCH_SET distinct partners, then partners reached through virtual chunks alone
        [(2, 5000 * j + 100, 5000 * j + 900, 800) for j in range(N_SINGLE)] +
        [(1, 10_000 * 100 + 300, 10_000 * 100 + 1300, 1000), (1, 10_000 * 3000 + 600, 10_000 * 3000 + 1600, 1000),
         (2, 5000 * 5 + 100, 5000 * 5 + 900, 800), (1, 10_000 * 120 + 300, 10_000 * 120 + 1300, 1000),
         (1, 10_000 * 200 + 600, 10_000 * 200 + 1600, 1000)] +
        [(2, 5000 * j + 100, 5000 * j + 900, 800) for j in range(N_SINGLE)][:40],
    ]
    return q


@pytest.fixture(scope='module')
def loaded():
    data, reads = resident()
    csr = data.csr()
    ctx = _lib.Context(0)
    ctx.load_csr_any(csr, fold_overlap_threshold(csr.iv_aln, PCT))
    ctx.build_index()
    assert ctx.n_reads > csr.n_reads and csr.n_reads <= 500
    ql = queries(reads)
    q = mr.Queries(ql, [1000] * len(ql), [4] * len(ql))
    yield ctx, data, csr, q, lr_rank(data)
    ctx.close()


def lr_rank(data):
    names = data.qnames[data.csr().read_qcode].tolist()
    return {int(name[1:]): r for r, name in enumerate(names)}


@pytest.mark.parametrize('emit', [0, SCORE_EDGE, SCORE_GATE, SCORE_ZD_OVERLAP])
def test_equals_the_reference(loaded, emit):
    ctx, data, csr, q, rank = loaded
    assert sorted(np.diff(q.off).tolist())[-1] == 4096 and {64, 65, 129} <= set(np.diff(q.off).tolist())
    want = ar.match_ref_any(data, csr, q, PCT, ar.CUTS, emit)
    got = run_any(ctx, data, q, ar.CUTS, emit, 4096)
    same(got, want, str(emit))
    if emit == 0:
        off, partner = got[0], got[1]
        for k in range(len(q)):                                  # a real read is one candidate per query read
            mine = partner[off[k]:off[k + 1]]
            assert np.unique(mine).size == mine.size
        longs = {rank[0], rank[1], rank[2]}
        assert longs <= set(partner[off[0]:off[1]].tolist()) and partner.max() < csr.n_reads
        assert got[5][6, 0] > MATCH_SET                          # the partner set closed
        assert {rank[1], rank[2]} <= set(partner[off[6]:off[7]].tolist()[MATCH_SET:])
        assert got[2].max() > 255 and (got[4] & SCORE_ZD_OVERLAP).any() and (got[4] & SCORE_EDGE).any()
        assert ((got[4] & SCORE_GATE) == 0).any()


def test_exclude_a_long_read(loaded):
    ctx, data, csr, q, rank = loaded
    qx = mr.Queries(q.reads, q.qlen2, q.nal, exclude=[rank[2]] * len(q))
    want = ar.match_ref_any(data, csr, qx, PCT, ar.CUTS, 0)
    got = run_any(ctx, data, qx, ar.CUTS, 0, 4096)
    same(got, want)
    assert rank[2] not in got[1].tolist()
    with pytest.raises(_lib.FslrError, match=f'fslr error {_lib.FSLR_ERR_INVALID}.*exclude'):
        run_any(ctx, data, q, ar.CUTS, 0, 4096, exclude=np.full(len(q), csr.n_reads, np.int32))   # a chunk's rank


def test_chunking(loaded, monkeypatch):
    ctx, data, csr, q, rank = loaded
    want = ar.match_ref_any(data, csr, q, PCT, ar.CUTS, SCORE_GATE)
    monkeypatch.setenv('FSLR_MATCH_BUDGET', '50')                # several chunks; single reads exceed it
    got = run_any(ctx, data, q, ar.CUTS, SCORE_GATE, 4096)
    same(got, want)
    again = run_any(ctx, data, q, ar.CUTS, SCORE_GATE, 4096)
    for x, y in zip(got, again):
        assert x.tobytes() == y.tobytes()


def test_too_long_and_missing_umax(loaded):
    ctx, data, csr, q, rank = loaded
    bad = mr.Queries([q.reads[5], [(1, 100 * k, 100 * k + 50, 50) for k in range(4097)]], [1000, 1000], [4, 4])
    with pytest.raises(_lib.FslrError, match=f'fslr error {_lib.FSLR_ERR_INVALID}.*query read 1 .*4097'):
        run_any(ctx, data, bad, ar.CUTS, 0, 4096, umax=umax_table(ar.CUTS, 4097))
    for um in (None, umax_table(ar.CUTS, 4095)):
        with pytest.raises(_lib.FslrError, match=f'fslr error {_lib.FSLR_ERR_INVALID}.*umax'):
            run_any(ctx, data, q, ar.CUTS, 0, 4096, umax=um)
    with pytest.raises(_lib.FslrError, match=f'fslr error {_lib.FSLR_ERR_STATE}'):
        ctx.match_rows()                                          # the old call does not read an _any batch


def test_tied_starts_without_data_positions():
    """Ties of equal (start, end) under an index uploaded without iv_data_pos that holds a long read: a tied
    hit ranks by its index in the real CSR.  The long read's tied intervals lie in its second chunk, which the
    virtual CSR stores behind every other read."""
    X = (1, 1000, 2000, 1000)
    reads = [[(3, 100 * k, 100 * k + 10, 10) for k in range(64)] + [X] * 6, [X, X], [(1, 1000, 2500, 1500), X], [X],
             [(1, 1000, 2000, 1000), (1, 900, 2000, 1100)], [X] * 3]
    data = ar.unsorted_data(reads, [1000] * 6, [4] * 6)
    csr = data.csr()
    assert not csr.start_sorted and np.array_equal(csr.data_pos, np.arange(csr.n_intervals))
    q = mr.Queries([[(1, 1500, 1600, 100)], [(1, 950, 1000, 50), (1, 1999, 2400, 401)], [X] * 70], [1000] * 3, [4] * 3)
    want = ar.match_ref_any(data, csr, q, PCT, ar.CUTS, 0)
    ctx = _lib.Context(0)
    try:
        ctx.load_csr_any(csr, fold_overlap_threshold(csr.iv_aln, PCT))
        ctx.build_index()
        got = run_any(ctx, data, q, ar.CUTS, 0, 70)
        same(got, want)
        assert got[1][:6].tolist() == want[1][:6].tolist() and want[1][0] != 0   # the long read is not met first
    finally:
        ctx.close()


def test_best_above_the_8_bit_range():
    """best between an I = 257, U = 300 edge and a later I = 250, U = 257 edge: the second is larger by exact
    comparison (250 * 300 > 257 * 257), while their low 8 bits (1 / 44 against 250 / 1) and a clamp to 255
    both say otherwise.  (Both edges of one query read have U >= its length >= 257, so no second edge of
    I = 200, U = 233 can exist beside the first.)"""
    reads = [ar.diag(257) + [(3, 100 * k, 100 * k + 10, 10) for k in range(43)], ar.diag(250)]
    # the 300-interval read must be met first: its extra intervals start before everything else
    data = mr.resident_data(reads, [1000, 1000], [4, 4])
    csr = data.csr()
    q = mr.Queries([ar.diag(257), list(reversed(ar.diag(257)))], [1000, 1000], [4, 4])
    cuts = [0.5]
    want = ar.match_ref_any(data, csr, q, PCT, cuts, 0)
    assert sorted(zip(want[2][:2].tolist(), want[3][:2].tolist())) == [(250, 257), (257, 300)]
    ctx = _lib.Context(0)
    try:
        ctx.load_csr_any(csr, fold_overlap_threshold(csr.iv_aln, PCT))
        ctx.build_index()
        got = run_any(ctx, data, q, cuts, 0, 300)
        same(got, want)
        short = int(np.flatnonzero(np.diff(csr.read_off) == 250)[0])
        assert got[6].tolist() == [short, short] and (got[4] & SCORE_EDGE).all()
    finally:
        ctx.close()


def test_short_only_equals_match_reads():
    s = synth.generate(1500, 16, 5)
    data = s.interval_data()
    csr = data.csr()
    lists = ar.lists_of(data, csr)
    rng = np.random.default_rng(2)
    pick = rng.choice(csr.n_reads, 300, replace=False)
    ql = [[(c, a + int(rng.integers(-3, 4)), b + int(rng.integers(-3, 4)), w) for c, a, b, w in lists[r]] for r in pick]
    q = mr.Queries(ql, csr.read_qlen2[pick], csr.read_nal[pick], exclude=pick)
    pt = pass_table(ar.CUTS)
    ctx = _lib.Context(0)
    try:
        ctx.load_csr_any(csr, fold_overlap_threshold(csr.iv_aln, PCT))
        ctx.build_index()
        for emit in (0, SCORE_EDGE):
            old = q.run(ctx, data, PCT, ar.QLEN_DIFF, ar.NAL_DIFF, pt, emit)
            new = run_any(ctx, data, q, ar.CUTS, emit, 16, umax=None)
            for x, y in zip(old, new):
                assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
        assert new[1].size > 100 and (new[6] >= 0).any()
        with pytest.raises(_lib.FslrError, match=f'fslr error {_lib.FSLR_ERR_STATE}'):
            ctx.match_rows()
        # a long query read on the short-only index
        big = mr.Queries([[x for r in pick[:40] for x in lists[r]][:129]], [1000], [4])
        assert len(big.reads[0]) == 129
        same(run_any(ctx, data, big, ar.CUTS, 0, 16), ar.match_ref_any(data, csr, big, PCT, ar.CUTS, 0))
    finally:
        ctx.close()


def test_index_method():
    data, reads = resident()
    idx = cluster.build_interval_trees(data)
    try:
        assert idx.long is not None
        new = mr.resident_data([[(c, s + 5, e + 5, a) for c, s, e, a in reads[1]], reads[10]], [1000, 1000], [4, 4])
        m = idx.match_reads_any(new, PCT, ar.CUTS, ar.QLEN_DIFF, ar.NAL_DIFF, emit='all')
        ncsr = new.csr()
        q = mr.Queries(ar.lists_of(new, ncsr), ncsr.read_qlen2, ncsr.read_nal)
        want = ar.match_ref_any(data, idx.csr, q, PCT, ar.CUTS, 0)
        same((m.offsets, m.partner, m.I, m.U, m.flags, m.counts, m.best), want)
        assert m.I.max() == 130
        with pytest.raises(NotImplementedError, match='64'):
            idx.match_reads(new, PCT, ar.CUTS, ar.QLEN_DIFF, ar.NAL_DIFF)
    finally:
        idx.ctx.close()
    with pytest.raises(NotImplementedError, match='multi-GPU'):
        cluster.MultiGpuIndex(data, 2).match_reads_any(new, PCT, ar.CUTS, ar.QLEN_DIFF, ar.NAL_DIFF)
