"""Matching new reads against the resident index on the device (fslr_match_reads / fslr_match_rows /
DeviceIntervalIndex.match_reads): rows, their order, the counts and the best partner against the CPU
expectation (match_ref), against the composed path (fslr_score_pairs after a second upload) and against
the clusterer itself, at the lane-group widths of score.hip, the piece / tile / group sizes of search.hip
and across the per-wave partner set's capacity."""
import ctypes

import numpy as np
import pytest

import match_ref as mr
from fslr_amd import _lib, cluster, synth
from fslr_amd._lib import MATCH_SET, SCORE_EDGE, SCORE_GATE, SCORE_ZD_GATE, SCORE_ZD_OVERLAP
from fslr_amd.prep import fold_overlap_threshold, pass_table

pytestmark = pytest.mark.gpu

CUTOFFS = (1, 1, 0.66, 0.66, 0.66, 0.5)
PCT, QD, ND = 0.8, 0.04, 0.25
PT = pass_table(CUTOFFS)
EMIT = {'edges': SCORE_EDGE, 'gated': SCORE_GATE, 'all': 0}
NAMES = ('offsets', 'partner', 'I', 'U', 'flags', 'counts', 'best')


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def load(ctx, data, pct=PCT):
    csr = data.csr()
    ctx.load_csr(csr, fold_overlap_threshold(csr.iv_aln, pct))
    ctx.build_index()
    return csr


def same(got, want, what=''):
    for name, g, w in zip(NAMES, got, want):
        np.testing.assert_array_equal(g, w, err_msg=f'{what} {name}')


# ------------------------------------------------------------------ 1. equality with match_ref
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64)


def dense_case():
    """Resident: six reads per length, dense on three chromosomes (a row has several candidate columns),
    some with an aln_size == 0 interval, some with qlen2 or n_alignments 0.  Queries: per length a jittered
    copy of a resident read (an edge) and a random read, with zeros of their own."""
    rng = np.random.default_rng(21)

    def read(L):
        s, w = rng.integers(5, 150, L), rng.integers(85, 115, L)
        return [(int(c), int(a), int(a + b), int(b)) for c, a, b in zip(rng.integers(3, 6, L), s, w)]
    reads, qlen2, nal = [], [], []
    for L in LENGTHS[1:]:
        for k in range(6):
            r = read(L)
            if k == 4:
                c, s, e, _ = r[L // 2]
                r[L // 2] = (c, s, e, 0)
            reads.append(r)
            qlen2.append(0 if k == 5 and L % 2 else int(rng.integers(980, 1020)))
            nal.append(0 if k == 5 else int(rng.integers(3, 5)))
    q, q2, qn = [], [], []
    for t, L in enumerate(LENGTHS):
        src = 6 * (t - 1)
        copy = [(c, s + int(rng.integers(-2, 3)), e + int(rng.integers(-2, 3)), a) for c, s, e, a in reads[src]] if L else []
        q += [copy, read(L)]
        q2 += [qlen2[src] if L else 1000, 0 if L in (15, 32) else 1000]
        qn += [nal[src] if L else 3, 0 if L in (15, 16) else 3]
    c, s, e, _ = q[9][3]                           # a query interval with aln_size == 0
    q[9][3] = (c, s, e, 0)
    return mr.resident_data(reads, qlen2, nal, shuffle_seed=4), mr.Queries(q, q2, qn)


@pytest.fixture(scope='module')
def dense(ctx):
    data, q = dense_case()
    return data, q, {e: mr.match_ref(data, data.csr(), q, PCT, QD, ND, PT, m) for e, m in EMIT.items()}


@pytest.mark.parametrize('emit', ['edges', 'gated', 'all'])
def test_equals_the_reference(ctx, dense, emit):
    data, q, want = dense
    load(ctx, data)
    got = q.run(ctx, data, PCT, QD, ND, PT, EMIT[emit])
    same(got, want[emit], emit)
    if emit == 'all':
        fl = got[4]
        for bit in (SCORE_GATE, SCORE_EDGE, SCORE_ZD_GATE, SCORE_ZD_OVERLAP):
            assert (fl & bit).any(), bit
        assert got[5][0].tolist() == [0, 0, 0] and got[6][0] == -1        # the 0-interval query reads
        assert (got[5][:, 0] == np.diff(got[0])).all() and got[5][2:, 0].min() > 10
        lens = np.diff(data.csr().read_off)[got[1]]
        assert set(LENGTHS[1:]) <= set(lens.tolist())                     # partners of every width were scored


def test_all_equals_the_composed_path(ctx, dense):
    """emit='all' against fslr_score_pairs on a second context that holds the resident reads with the
    query reads appended (the path a caller had to compose before)."""
    data, q, _ = dense
    csr = load(ctx, data)
    off, partner, I, U, flags, _, _ = q.run(ctx, data, PCT, QD, ND, PT, 0)
    keep = np.flatnonzero(np.diff(q.off) > 0)            # an upload takes no empty read
    n = csr.n_reads
    qlen = np.diff(q.off)
    sel = np.concatenate([np.arange(q.off[k], q.off[k + 1]) for k in keep])
    read_off = np.concatenate([csr.read_off, csr.read_off[-1] + np.cumsum(qlen[keep])])
    c2 = _lib.Context(0)
    try:
        c2.set_reads(read_off, np.concatenate([csr.read_qlen2, q.qlen2[keep]]), np.concatenate([csr.read_nal, q.nal[keep]]),
                     np.concatenate([csr.iv_chrom, q.dense_chrom(data)[sel]]),
                     np.concatenate([csr.iv_start, q.flat[sel, 1]]), np.concatenate([csr.iv_end, q.flat[sel, 2]]),
                     np.concatenate([fold_overlap_threshold(csr.iv_aln, PCT), fold_overlap_threshold(q.flat[sel, 3], PCT)]),
                     csr.n_chroms)
        new_rank = np.full(len(q), -1)
        new_rank[keep] = n + np.arange(keep.size)
        a = new_rank[np.repeat(np.arange(len(q)), np.diff(off))]
        assert a.size > 500 and a.min() >= n
        I2, U2, f2 = c2.score_pairs(a, partner, 1 - QD, 1 - ND, PT)
    finally:
        c2.close()
    for g, w in ((I, I2), (U, U2), (flags, f2)):
        np.testing.assert_array_equal(g, w)


# ------------------------------------------------------------------ 2. the seen-set
def ladder_case():
    """Chromosome 1: read k holds [10 k, 10 k + 5] and [10 k + 2, 10 k + 8], so a query interval [0, x] takes
    any number of hits and two intervals of one partner.  Chromosome 2: 300 single-interval reads of one start
    (the order inside the run decides the candidate order)."""
    rng = np.random.default_rng(6)
    reads = [[(1, 10 * k, 10 * k + 5, 5), (1, 10 * k + 2, 10 * k + 8, 6)] for k in range(1100)]
    reads += [[(2, 1000, 1000 + int(e), int(e))] for e in rng.integers(1, 60, 300)]
    data = mr.resident_data(reads, np.full(len(reads), 1000), np.full(len(reads), 3), shuffle_seed=9)
    starts = np.sort(np.array([iv[1] for r in reads[:1100] for iv in r]))
    q = [[(1, 0, 10 * d - 1, 100)] for d in (MATCH_SET - 1, MATCH_SET, MATCH_SET + 1, 2 * MATCH_SET + 3)]
    hit_counts = (63, 64, 65, 255, 256, 257, 1500)
    q += [[(1, 0, int(starts[h - 1]), 100)] for h in hit_counts]
    # partners met again by later intervals, past the set's capacity; then the run of equal start, twice
    q.append([(1, 2000, 5000, 100), (1, 0, 4000, 100), (2, 1000, 1030, 30), (1, 3000, 9000, 100), (1, 0, 12000, 100)])
    q.append([(2, 1000, 1010, 10), (2, 990, 1100, 100), (1, 5, 5, 1)])
    return data, mr.Queries(q, np.full(len(q), 1000), np.full(len(q), 3)), hit_counts


def test_seen_set_and_search_sizes(ctx):
    data, q, hit_counts = ladder_case()
    csr = load(ctx, data)
    cands, hits = mr.candidates(data, csr, q)
    assert [c.size for c in cands[:4]] == [MATCH_SET - 1, MATCH_SET, MATCH_SET + 1, 2 * MATCH_SET + 3]
    assert tuple(hits[4:11]) == hit_counts
    assert hits[11] > 2 * cands[11].size > 4 * MATCH_SET and cands[12].size == 301
    want = mr.match_ref(data, csr, q, PCT, QD, ND, PT, 0)
    got = q.run(ctx, data, PCT, QD, ND, PT, 0)
    same(got, want)
    assert got[5][:, 0].tolist() == [c.size for c in cands]


# ------------------------------------------------------------------ 3. the clusterer itself
def test_consistent_with_the_clusterer(ctx):
    """Every resident read of a synth set as the query with exclude = itself: among partners of higher rank
    exactly the walk engine's edges with its I | U << 8, the candidate counts sum to its evaluated_pairs,
    and the rows to lower ranks equal fslr_score_pairs(a = q, b = partner)."""
    csr = synth.generate(2000, 16, 11).interval_data().csr()
    n = csr.n_reads
    thr = fold_overlap_threshold(csr.iv_aln, PCT)
    ctx.load_csr(csr, thr)
    ctx.reserve_edges(1 << 16)
    ctx.build_index()
    st = ctx.run_query(1 - QD, 1 - ND, PT, edge_threshold=1 << 30, engine='walk')
    assert st['engine'] == 'walk'
    ea, eb, eI, eU = ctx.edges(st['n_edges'])
    off, counts, best = ctx.match_reads(csr.read_off, csr.read_qlen2, csr.read_nal, csr.iv_chrom, csr.iv_start,
                                        csr.iv_end, thr, 1 - QD, 1 - ND, PT, 0, np.arange(n))
    partner, I, U, flags = ctx.match_rows()
    qi = np.repeat(np.arange(n), np.diff(off))
    assert (partner != qi).all()
    up = (partner > qi) & ((flags & SCORE_EDGE) != 0)
    got = sorted(zip(qi[up].tolist(), partner[up].tolist(), (I[up] | U[up] << 8).tolist()))
    want = sorted(zip(ea.tolist(), eb.tolist(), (eI.astype(np.int64) | eU.astype(np.int64) << 8).tolist()))
    assert len(want) >= 1000 and got == want
    assert int((partner > qi).sum()) == st['evaluated_pairs'] == int(counts[:, 0].sum()) // 2
    down = partner < qi
    I2, U2, f2 = ctx.score_pairs(qi[down], partner[down], 1 - QD, 1 - ND, PT)
    for g, w in ((I[down], I2), (U[down], U2), (flags[down], f2)):
        np.testing.assert_array_equal(g, w)
    assert (counts[:, 2] == np.bincount(qi[(flags & SCORE_EDGE) != 0], minlength=n)).all()


# ------------------------------------------------------------------ 4. chunking
def test_chunks_give_the_same_bytes(ctx, monkeypatch):
    data, q, _ = ladder_case()
    load(ctx, data)
    one = q.run(ctx, data, PCT, QD, ND, PT, 0)
    _, hits = mr.candidates(data, data.csr(), q)
    budget = 1200
    assert max(hits) > budget and sum(hits) >= 5 * budget              # >= 5 chunks, one read alone past the budget
    monkeypatch.setenv('FSLR_MATCH_BUDGET', str(budget))
    same(q.run(ctx, data, PCT, QD, ND, PT, 0), one, 'chunked')
    monkeypatch.setenv('FSLR_MATCH_BUDGET', '1')                       # every read a chunk
    same(q.run(ctx, data, PCT, QD, ND, PT, SCORE_GATE), q.run(ctx, data, PCT, QD, ND, PT, 0), 'gated')
    monkeypatch.delenv('FSLR_MATCH_BUDGET')
    same(q.run(ctx, data, PCT, QD, ND, PT, 0), one, 'again')           # two runs, identical bytes


# ------------------------------------------------------------------ 5. contract
def raw_call(ctx, off, nq, chrom, start, end, thr, excl=None):
    a = [np.ascontiguousarray(x, np.int32) for x in (off, np.full(nq, 1000), np.full(nq, 3), chrom, start, end, thr)]
    q = _lib.MatchQueries(nq, a[3].size, *(_lib._ptr(x) for x in a), None)
    p = ctx._params(1 - QD, 1 - ND, PT, 0)
    total = ctypes.c_int64(-7)
    rc = ctx._L.fslr_match_reads(ctx._h, ctypes.byref(p), ctypes.byref(q), 0, None, None, None, ctypes.byref(total))
    return rc, total.value, (ctx._L.fslr_last_error(ctx._h) or b'').decode()


def test_contract(ctx):
    data, q, _ = ladder_case()
    csr = load(ctx, data)
    # no query read; a chromosome id out of range has no hits
    off, counts, best = ctx.match_reads([0], [], [], [], [], [], [], 1 - QD, 1 - ND, PT)
    assert off.tolist() == [0] and counts.shape == (0, 3) and best.size == 0 and ctx.match_rows()[0].size == 0
    off, counts, best = ctx.match_reads([0, 2], [1000], [3], [csr.n_chroms, -1], [0, 0], [9000, 9000], [1, 1],
                                        1 - QD, 1 - ND, PT, 0)
    assert off.tolist() == [0, 0] and counts.tolist() == [[0, 0, 0]] and best.tolist() == [-1]
    # 65 intervals, a decreasing read_off: FSLR_ERR_INVALID naming the read
    z = np.zeros(66, np.int32)
    rc, total, msg = raw_call(ctx, [0, 1, 66], 2, z, z, z + 5, z + 1)
    assert rc == _lib.FSLR_ERR_INVALID and 'query read 1' in msg and '65' in msg and total == -7
    rc, total, msg = raw_call(ctx, [0, 2, 1], 2, z[:2], z[:2], z[:2] + 5, z[:2] + 1)
    assert rc == _lib.FSLR_ERR_INVALID and 'query read 1' in msg
    # a short capacity writes nothing
    got = q.run(ctx, data, PCT, QD, ND, PT, 0)
    n = got[1].size
    bufs = [np.full(n, -7, np.int32) for _ in range(3)] + [np.full(n, 77, np.uint8)]
    rc = ctx._L.fslr_match_rows(ctx._h, *(_lib._ptr(b) for b in bufs), n - 1)
    assert rc == _lib.FSLR_ERR_INVALID and str(n) in ctx._L.fslr_last_error(ctx._h).decode()
    assert all((b == (77 if b.dtype == np.uint8 else -7)).all() for b in bufs)
    assert ctx._L.fslr_match_rows(ctx._h, *(_lib._ptr(b) for b in bufs), n) == _lib.FSLR_OK
    same(bufs, got[1:5])
    # the saved batch belongs to the index build it was made on
    ctx.build_index()
    with pytest.raises(_lib.FslrError, match=f'fslr error {_lib.FSLR_ERR_STATE}.*fslr_match_reads first'):
        ctx.match_rows()


def test_state_errors():
    data, q, _ = ladder_case()
    csr = data.csr()
    c = _lib.Context(0)
    try:
        c.load_csr(csr, fold_overlap_threshold(csr.iv_aln, PCT))
        with pytest.raises(_lib.FslrError, match=f'fslr error {_lib.FSLR_ERR_STATE}.*fslr_build_index'):
            q.run(c, data, PCT, QD, ND, PT, 0)
        owned = np.zeros(csr.n_chroms, np.uint8)
        owned[0] = 1
        c.set_chrom_filter(owned)
        c.build_index()
        with pytest.raises(_lib.FslrError, match=f'fslr error {_lib.FSLR_ERR_STATE}.*filter'):
            q.run(c, data, PCT, QD, ND, PT, 0)
    finally:
        c.close()
    rng = np.random.default_rng(44)
    import search_ref as sr
    n = 400
    qcode = np.concatenate([np.zeros(70, np.int64), 1 + rng.integers(0, 100, n - 70)])
    start = rng.integers(0, 200, n) * 500
    long_data = sr.make_data(rng.integers(1, 3, n), start, start + rng.integers(50, 2500, n), qcode=qcode)
    idx = cluster.build_interval_trees(long_data)
    try:
        with pytest.raises(_lib.FslrError, match=f'fslr error {_lib.FSLR_ERR_INVALID}.*64'):
            idx.ctx.match_reads([0, 1], [1000], [3], [0], [0], [500], [1], 1 - QD, 1 - ND, PT)
        with pytest.raises(NotImplementedError, match='64'):
            idx.match_reads(sr.make_data([1], [0], [500]), PCT, CUTOFFS, QD, ND)
    finally:
        idx.ctx.close()


def test_other_state_is_left_alone(ctx):
    csr = synth.generate(2000, 16, 11).interval_data().csr()
    thr = fold_overlap_threshold(csr.iv_aln, PCT)
    ctx.load_csr(csr, thr)
    ctx.reserve_edges(1 << 16)
    ctx.build_index()
    st = ctx.run_query(1 - QD, 1 - ND, PT)
    ctx.components()
    ctx.cluster_table()

    def state():
        return (*ctx.edges(st['n_edges']), ctx.labels(), ctx.fwd_degree(), *ctx.cluster_ids(), *ctx.cluster_members())
    before = state()
    qs = (csr.iv_chrom[:300], csr.iv_start[:300], csr.iv_end[:300])
    want_off, want_hits = ctx.search(*qs)
    total = ctx._search(*qs, None)
    off, counts, best = ctx.match_reads(csr.read_off, csr.read_qlen2, csr.read_nal, csr.iv_chrom, csr.iv_start,
                                        csr.iv_end, thr, 1 - QD, 1 - ND, PT, SCORE_EDGE, np.arange(csr.n_reads))
    assert off[-1] == 2 * st['n_edges'] > 1000 and ctx.match_rows()[0].size == off[-1]
    hits = np.full(total, -7, np.int32)
    ctx._check(ctx._L.fslr_search_hits(ctx._h, _lib._ptr(hits), total))     # the saved search batch survived
    np.testing.assert_array_equal(hits, want_hits)
    for x, y in zip(before, state()):
        np.testing.assert_array_equal(x, y)


def rows_index(data):
    """The resident reads staged from rows on the device (fslr_rows_upload / fslr_set_reads_rows), as the
    columnar CLI stages them; ``data`` is start-sorted, so the start order is the identity."""
    c = _lib.Context(0)
    rows = dict(chrom=data.chrom, start=data.start, end=data.end, aln=data.aln_size, qcode=data.qcode,
                nal=data.n_alignments, qlen2=data.qlen2)
    c.rows_upload({k: np.ascontiguousarray(v, np.int64) for k, v in rows.items()}, len(data.qnames),
                  int(data.chrom.max()) + 1)
    info = c.set_reads_rows(np.arange(len(data), dtype=np.int64), None, PCT)
    return cluster.RowsIndex(data, cluster.RowsCSR(c, info), c, PCT)


def test_index_methods(ctx):
    """DeviceIntervalIndex.match_reads on new reads drawn from the resident set's own events: the same
    rows as the binding gives for their CSR, qnames in the frame, clusters from the labels; and the same
    through a RowsIndex staged with fslr_set_reads_rows."""
    s = synth.generate(2200, 16, 11)
    data = s.interval_data()
    csr_all = data.csr()
    new_ranks = np.arange(0, csr_all.n_reads, 11)
    is_new = np.isin(np.repeat(np.arange(csr_all.n_reads), np.diff(csr_all.read_off)), new_ranks)
    new_pos = np.zeros(len(data), bool)
    new_pos[np.asarray(csr_all.data_pos, np.int64)] = is_new
    resident, new = data.select(~new_pos), data.select(new_pos)
    idx = cluster.build_interval_trees(resident, ctx=ctx)
    m = idx.match_reads(new, PCT, CUTOFFS, QD, ND)
    assert len(m) == new_ranks.size and (m.flags & SCORE_EDGE).all() and m.partner.size > 100
    assert (m.counts[:, 2] == np.diff(m.offsets)).all()
    qc = new.csr()
    want = mr.match_ref(resident, idx.csr, mr.Queries(
        [[(int(new.chrom[k]), int(new.start[k]), int(new.end[k]), int(new.aln_size[k]))
          for k in np.asarray(qc.data_pos[qc.read_off[r]:qc.read_off[r + 1]], np.int64)] for r in range(40)],
        qc.read_qlen2[:40], qc.read_nal[:40]), PCT, QD, ND, PT, SCORE_EDGE)
    k = int(want[0][-1])
    assert k > 10
    same([x[:k] for x in (m.partner, m.I, m.U, m.flags)], want[1:5])
    np.testing.assert_array_equal(m.offsets[:41], want[0])
    f = m.to_frame()
    assert f.shape == (m.partner.size, 4) and f['query'].iloc[0] == new.qnames[qc.read_qcode][m.query_of_row()[0]]
    assert f['qname'].iloc[0] == resident.qnames[idx.csr.read_qcode][m.partner[0]]
    labels = np.arange(idx.csr.n_reads)                                     # every read its own component
    off, lab, join = m.clusters(labels)
    assert (np.diff(off) == m.counts[:, 2]).all() and (lab == m.partner).all()
    everything = idx.match_reads(new, PCT, CUTOFFS, QD, ND, emit='all')
    assert (np.diff(everything.offsets) == m.counts[:, 0]).all() and everything.partner.size > m.partner.size
    # the same resident reads staged from rows on the device
    ridx = rows_index(resident)
    try:
        assert isinstance(ridx, cluster.RowsIndex)
        r = ridx.match_reads(new, PCT, CUTOFFS, QD, ND)
        names = ridx.data.qnames[ridx.csr.read_qcode]
        got = sorted(zip(r.query_of_row().tolist(), names[r.partner].tolist(), r.I.tolist(), r.U.tolist()))
        mine = resident.qnames[idx.csr.read_qcode]
        assert got == sorted(zip(m.query_of_row().tolist(), mine[m.partner].tolist(), m.I.tolist(), m.U.tolist()))
    finally:
        ridx.ctx.close()
