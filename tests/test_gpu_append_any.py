"""fslr_append_reads_any / DeviceIntervalIndex.append with reads of more than 64 intervals.

The yardstick of every case is a FRESH context given fslr_set_reads_any of the union's real CSR
(append_ref.concat_csr: the resident reads, then the batch, with the merged data positions).  Both contexts then
build their index and answer the same questions: the query (edges with I and U, the long-pair edges, forward
degrees and labels through cluster._query_long, which installs the thresholds in REAL interval order and the
cutoff table first), a search batch (its order shows the merged data order), score_pairs_any on pairs that name
the moved chunk reads, and match_reads_any through the wrapper.  Everything is compared exactly."""
import ctypes
import types
import warnings

import numpy as np
import pytest

import append_ref as ar
import match_ref as mr
from host_pipeline import host_prepare
from fslr_amd import _lib, cluster
from fslr_amd._lib import FSLR_ERR_INVALID, FSLR_ERR_STATE
from fslr_amd.prep import has_long_reads, pass_table, remove_reads_csr, split_long_reads, umax_table
from oracle import oracle as O
from test_gpu_parity import oracle_from_csr
from test_gpu_append import CUTOFFS, ND, PCT, QD, graph, one_locus, rebased, same_search, thr_of

pytestmark = pytest.mark.gpu

PT = pass_table(CUTOFFS)


@pytest.fixture
def ctxs():
    a, b = _lib.Context(0), _lib.Context(0)
    yield a, b
    a.close()
    b.close()


def long_read(L, start0, step=7, width=60, chrom=1):
    return [(chrom, start0 + step * k, start0 + step * k + width, width) for k in range(L)]


def data_of(reads, seed):
    n = len(reads)
    rng = np.random.default_rng(seed)
    return mr.resident_data(reads, rng.integers(950, 1050, n), np.full(n, 3), shuffle_seed=seed)


def case(res_reads, *batches, seed=1):
    """(resident CSR, rebased batch CSRs ...) of read lists."""
    res_d = data_of(res_reads, seed)
    res = res_d.csr()
    return (res,) + tuple(rebased(res_d, res, data_of(b, seed + 1 + t)) for t, b in enumerate(batches))


def load(ctx, csr, pct=PCT):
    (ctx.load_csr_any if has_long_reads(csr) else ctx.load_csr)(csr, thr_of(csr, pct))


def results(ctx, csr, edge_threshold=10, pct=PCT):
    """The query's answers on a context that holds ``csr`` (a real CSR)."""
    ctx.build_index()
    if not has_long_reads(csr):
        ctx.set_thresholds(thr_of(csr, pct))
        g = graph(ctx, csr.n_reads, edge_threshold=edge_threshold)
        return dict(edges=g['edges'], fwd=g['fwd'].tolist(), labels=g['labels'].tolist(), engine=g['counts']['engine'])
    idx = types.SimpleNamespace(csr=csr, ctx=ctx, long=np.diff(csr.read_off).astype(np.int32), data=None)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', cluster.EdgeCapWarning)
        try:
            g = cluster._query_long(idx, pct, list(CUTOFFS), edge_threshold, QD, ND)
        except ZeroDivisionError:                           # the reference raises too (an aln_size == 0 interval is met)
            st = ctx.stats(check=False)
            return dict(raised=True, zd_pairs=st['zd_pairs'], n_edges=st['n_edges'])
    return dict(edges=sorted(zip(g.a.tolist(), g.b.tolist(), g.I.tolist(), g.U.tolist())), fwd=np.asarray(g.fwd).tolist(),
                labels=np.asarray(g.labels).tolist(), engine=g.stats['engine'], cap=g.stats['cap'],
                long_pair_edges=g.stats['long_pair_edges'])


def scores(ctx, csr, seed=0):
    """score_pairs_any on pairs that name every long read (its chunks moved) and a sample of the others."""
    n = csr.n_reads
    L = np.diff(csr.read_off)
    rng = np.random.default_rng(seed)
    lg = np.flatnonzero(L > 64)
    a = np.concatenate([np.repeat(lg, 8), rng.integers(0, n, 200)])
    b = np.concatenate([rng.integers(0, n, 8 * lg.size), rng.integers(0, n, 200)])
    ok = a != b
    I, U, fl = ctx.score_pairs_any(a[ok], b[ok], 1 - QD, 1 - ND, PT, umax=umax_table(list(CUTOFFS), int(L.max())))
    return I.tolist(), U.tolist(), fl.tolist()


def match_rows(ctx, csr, pct=PCT):
    """fslr_match_reads_any with the long reads of at most 300 intervals and every seventh read of ``csr`` as query
    reads, 60 at the most (no exclusion, every candidate emitted; longer reads are partners only, which keeps the
    case quick): offsets, counts, best and the rows.  The context's thresholds are folded for ``pct``."""
    L = np.diff(csr.read_off)
    pick = ((L > 64) & (L <= 300)) | (np.arange(csr.n_reads) % 7 == 0)
    pick &= np.cumsum(pick) <= 60
    q, _ = remove_reads_csr(csr, pick)
    off, counts, best = ctx.match_reads_any(q.read_off, q.read_qlen2, q.read_nal, q.iv_chrom, q.iv_start, q.iv_end,
                                            thr_of(q, pct), 1 - QD, 1 - ND, PT, 0, None,
                                            umax=umax_table(list(CUTOFFS), int(L.max())))
    return [np.asarray(x).tolist() for x in (off, counts, best) + tuple(ctx.match_rows_any())]


def same(ca, cb, u, what='', edge_threshold=10, pct=PCT):
    g, w = results(ca, u, edge_threshold, pct), results(cb, u, edge_threshold, pct)
    assert g == w, what
    same_search(ca, cb, u, what)
    assert scores(ca, u) == scores(cb, u), what
    ra, rb = match_rows(ca, u, pct), match_rows(cb, u, pct)
    assert len(ra[3]) > 0 and ra == rb, what
    return g


def append_vs_fresh(ctxs, res, batches, what='', edge_threshold=10, pct=PCT, built=True):
    ca, cb = ctxs
    load(ca, res, pct)
    if built:
        ca.build_index()
    u = res
    for bt in batches:
        ca.append_csr_any(bt, thr_of(bt, pct))
        u = ar.concat_csr(u, bt, n_chroms=bt.n_chroms)
    vn = split_long_reads(u)[0].n_reads if has_long_reads(u) else u.n_reads
    assert ca.n_reads == vn and ca.n_intervals == u.n_intervals
    load(cb, u, pct)
    return same(ca, cb, u, what, edge_threshold, pct), u


def locus(n, rng, lo=0, hi=3000, chrom=1):
    """Short reads of 1-3 intervals over [lo, hi)."""
    return [[(chrom, int(s), int(s) + 60, 60) for s in np.sort(rng.integers(lo, hi, int(rng.integers(1, 4))))] for _ in range(n)]


# ------------------------------------------------------------------ 1. the seams of the read length
def test_plain_resident_set_turns_virtual_on_a_65_interval_read(ctxs):
    rng = np.random.default_rng(1)
    res, bt = case(locus(300, rng), locus(40, rng) + [long_read(65, 100)] + locus(10, rng))
    assert not has_long_reads(res) and np.diff(bt.read_off).max() == 65
    g, u = append_vs_fresh(ctxs, res, [bt])
    assert g['engine'] in ('sweep+long', 'pairs') and len(g['edges']) > 0


def test_resident_chunks_move_behind_a_batch_of_short_reads(ctxs):
    """Resident long reads of 65, 128, 129 and 4096 intervals, a batch of short reads only: every resident
    chunk's rank and CSR rows move and no chunk is added."""
    rng = np.random.default_rng(2)
    res_reads = locus(200, rng) + [long_read(65, 50), long_read(128, 400), long_read(129, 400)] + locus(50, rng) + \
        [long_read(4096, 100000, step=1, width=40)]              # away from the query reads of match_rows: it only moves
    res, bt = case(res_reads, locus(120, rng))
    assert not has_long_reads(bt)
    g, u = append_vs_fresh(ctxs, res, [bt])
    assert g['long_pair_edges'] > 0


def test_long_reads_on_both_sides_and_two_appends_in_a_row(ctxs):
    rng = np.random.default_rng(3)
    res, b1, b2 = case(locus(200, rng) + [long_read(70, 10), long_read(200, 300, step=4)],
                       locus(60, rng) + [long_read(190, 300, step=4), long_read(66, 1500)],
                       [long_read(64, 700), long_read(65, 800)] + locus(30, rng))
    g, u = append_vs_fresh(ctxs, res, [b1, b2])
    assert np.diff(u.read_off).max() == 200 and g['long_pair_edges'] > 0


def test_batch_reads_of_exactly_64_and_of_the_limit(ctxs):
    rng = np.random.default_rng(4)
    res, bt = case(locus(150, rng) + [long_read(65, 20)], [long_read(64, 40), long_read(4096, 0, step=1, width=30)] + locus(20, rng))
    append_vs_fresh(ctxs, res, [bt])


@pytest.mark.parametrize('built', [False, True])
def test_new_chromosomes_and_buffers_that_grow(ctxs, built):
    """A batch larger than the resident set, on chromosomes the context has not seen: every buffer grows, with and
    without an index built on the old ones."""
    rng = np.random.default_rng(5)
    res, bt = case(locus(40, rng) + [long_read(100, 0)],
                   locus(300, rng, chrom=2) + [long_read(150, 5, chrom=3), long_read(90, 50, chrom=1)] + locus(200, rng, chrom=1))
    assert bt.n_chroms == res.n_chroms + 2
    append_vs_fresh(ctxs, res, [bt], built=built)


# ------------------------------------------------------------------ 2. the seams of the merge
def test_chunk_intervals_in_copy_tiles_mixed_tiles_and_across_a_tile_boundary(ctxs):
    """Starts arranged over the merge's 1024-output tiles: the resident long read's further chunks (starts from
    3000 on) lie in tiles the batch does not touch (a straight copy, tags moved), in tiles it shares with batch
    intervals (mixed), and one run of equal starts holds a resident chunk interval and a new interval."""
    rng = np.random.default_rng(6)
    long_res = [(1, 3000 + 2 * k, 3060 + 2 * k, 60) for k in range(64)] + [(1, 3000 + 2 * k, 3060 + 2 * k, 60) for k in range(64, 2600)]
    res_reads = locus(400, rng, 0, 2500) + [long_res]
    tie = 3000 + 2 * 1500                                         # the start of resident chunk interval 1500
    new_reads = [[(1, int(s), int(s) + 60, 60)] for s in rng.integers(4000, 4400, 300)] + [[(1, tie, tie + 60, 60)]] * 3 + \
        [long_read(80, 7000, step=2)]
    res, bt = case(res_reads, new_reads)
    (g, u) = append_vs_fresh(ctxs, res, [bt])
    starts = np.sort(u.iv_start)
    assert starts.size > 3 * 1024
    # the search order puts the new interval of the tie run before the resident one (descending data position)
    ca = ctxs[0]
    _, hits = ca.search(np.full(1, u.iv_chrom[-1], np.int32), np.full(1, tie, np.int32), np.full(1, tie, np.int32))
    tied = hits[u.iv_start[hits] == tie]
    assert tied.size == 4 and (tied[:3] >= res.n_intervals).all() and tied[3] < res.n_intervals


# ------------------------------------------------------------------ 3. cap and overlap 0
def dense_split(rng):
    """A dense locus with long reads (every read overlaps many): split into resident + batch."""
    reads = [long_read(int(L), int(s), step=3, width=80) for L, s in zip(rng.integers(1, 90, 60), rng.integers(0, 200, 60))]
    reads += [long_read(140, 10, step=3, width=80)]
    return reads[:40] + [reads[-1]], reads[40:-1]


def test_a_binding_cap_on_a_dense_long_read_locus(ctxs):
    res, bt = case(*dense_split(np.random.default_rng(7)))
    g, u = append_vs_fresh(ctxs, res, [bt], edge_threshold=3)
    assert g['cap']['applied'] == 1


def test_overlap_zero_takes_the_general_path(ctxs):
    res, bt = case(*dense_split(np.random.default_rng(8)))
    g, u = append_vs_fresh(ctxs, res, [bt], pct=0.0)
    assert g['engine'] == 'pairs'


# ------------------------------------------------------------------ 4. refusals
def raw_append_any(ctx, bt, thr):
    arrs = [np.ascontiguousarray(x, dtype=np.int32) for x in
            (bt.read_off, bt.read_qlen2, bt.read_nal, bt.iv_chrom, bt.iv_start, bt.iv_end, thr, bt.data_pos)]
    r = _lib.Reads(bt.n_reads, bt.n_intervals, int(bt.n_chroms), *(a.ctypes.data_as(ctypes.c_void_p) for a in arrs))
    rc = ctx._L.fslr_append_reads_any(ctx._h, ctypes.byref(r))
    return rc, (ctx._L.fslr_last_error(ctx._h) or b'').decode()


def saved_search(ctx, like):
    out = np.empty_like(like)
    return ctx._L.fslr_search_hits(ctx._h, out.ctypes.data_as(ctypes.c_void_p), out.size), out


class Intact:
    """A built index, a saved search batch and a saved match batch on ``ctx``; ``check()`` after a refused call: the
    saved batches read back the same and the index (not rebuilt) answers the same."""

    def __init__(self, ctx, csr, any_length=True):
        self.ctx, self.q = ctx, (csr.iv_chrom[:20], csr.iv_start[:20], csr.iv_end[:20])
        self.any = any_length
        ctx.build_index()
        k = csr.read_off[3]
        self.m = (csr.read_off[:4], csr.read_qlen2[:3], csr.read_nal[:3], csr.iv_chrom[:k], csr.iv_start[:k], csr.iv_end[:k],
                  thr_of(csr)[:k], 1 - QD, 1 - ND, PT, 0, None)
        self.rows = self.match()
        _, self.hits = ctx.search(*self.q)

    def match(self):
        if self.any:
            self.ctx.match_reads_any(*self.m, umax=umax_table(list(CUTOFFS), 4096))
            return [x.tolist() for x in self.ctx.match_rows_any()]
        self.ctx.match_reads(*self.m)
        return [x.tolist() for x in self.ctx.match_rows()]

    def check(self, fresh_search=True):
        ctx = self.ctx
        saved = [x.tolist() for x in (ctx.match_rows_any() if self.any else ctx.match_rows())]
        assert saved == self.rows and len(saved[0]) > 0
        rc, again = saved_search(ctx, self.hits)
        assert rc == 0
        np.testing.assert_array_equal(again, self.hits)
        if fresh_search:                                         # the index is still built: no build_index here
            np.testing.assert_array_equal(ctx.search(*self.q)[1], self.hits)


def saved(ctx, state):
    """What the saved search and match batches read back as right now (return code and rows), whatever their state."""
    rc, hits = saved_search(ctx, state.hits)
    try:
        rows = [x.tolist() for x in ctx.match_rows_any()]
    except _lib.FslrError as e:
        rows = str(e)
    return rc, hits.tolist() if rc == 0 else None, rows


def rows_context(ctx):
    n = 6
    cols = dict(chrom=np.ones(n), start=np.arange(n) * 5, end=np.arange(n) * 5 + 40, aln=np.full(n, 40),
                qcode=np.arange(n) // 2, nal=np.full(n, 3), qlen2=np.full(n, 1000))
    ctx.rows_upload(cols, 3, 2)
    ctx.set_reads_rows(np.arange(n), None, PCT)
    ctx.build_index()
    q = (np.zeros(3, np.int32), np.zeros(3, np.int32), np.full(3, 100, np.int32))
    _, hits = ctx.search(*q)
    return q, hits


def test_refusals_leave_the_index_and_the_saved_batches(ctxs):
    ca, _ = ctxs
    rng = np.random.default_rng(9)
    res, good, too_long = case(locus(100, rng) + [long_read(70, 10)], locus(10, rng) + [long_read(66, 5)],
                               [long_read(4097, 0, step=1, width=10)])
    load(ca, res)
    want = results(ca, res)
    state = Intact(ca, res)
    rc, text = raw_append_any(ca, too_long, thr_of(too_long))
    assert rc == FSLR_ERR_INVALID and 'FSLR_MAX_ANY_L' in text and '4097' in text, text
    state.check()
    ca.set_chrom_filter(np.ones(res.n_chroms, bool))
    before = saved(ca, state)                                    # (fslr_search itself refuses under a filter)
    rc, text = raw_append_any(ca, good, thr_of(good))
    assert rc == FSLR_ERR_STATE and 'filter' in text
    assert saved(ca, state) == before                            # the saved batches as the filter left them
    ca.set_chrom_filter(None)
    assert results(ca, res) == want                              # the reads are the ones that were there
    # virtual reads the caller made itself (fslr_set_long_reads): their real CSR is not known to the library
    v, vreal, vbase, rlen = split_long_reads(res)
    ca.load_csr(v, thr_of(v))
    ca.set_long_reads(res.n_reads, vreal, vbase, rlen, umax_table(list(CUTOFFS), int(rlen.max())))
    own = Intact(ca, res)
    rc, text = raw_append_any(ca, good, thr_of(good))
    assert rc == FSLR_ERR_STATE and 'fslr_set_long_reads' in text, text
    own.check()
    # rows-made reads
    q, hits = rows_context(ca)
    rc, text = raw_append_any(ca, good, thr_of(good))
    assert rc == FSLR_ERR_STATE and 'rows' in text
    rc, again = saved_search(ca, hits)
    assert rc == 0
    np.testing.assert_array_equal(again, hits)
    np.testing.assert_array_equal(ca.search(*q)[1], hits)
    load(ca, res)                                                # and the good batch still goes in
    rc, text = raw_append_any(ca, good, thr_of(good))
    assert rc == 0, text


# ------------------------------------------------------------------ 5. plain + short is fslr_append_reads
def test_a_plain_context_and_a_short_batch_take_the_short_path(ctxs):
    ca, cb = ctxs
    rng = np.random.default_rng(10)
    res, bt = case(locus(300, rng), locus(80, rng))
    ca.load_csr(res, thr_of(res))
    cb.load_csr(res, thr_of(res))
    ca.append_csr_any(bt, thr_of(bt))
    cb.append_csr(bt, thr_of(bt))
    u = ar.concat_csr(res, bt, n_chroms=bt.n_chroms)
    assert ca.n_reads == cb.n_reads == u.n_reads
    assert results(ca, u) == results(cb, u)
    same_search(ca, cb, u)


# ------------------------------------------------------------------ 6. determinism
def test_two_runs_give_the_same_bytes(ctxs):
    rng = np.random.default_rng(11)
    res, bt = case(locus(200, rng) + [long_read(129, 30), long_read(300, 500, step=3)], locus(80, rng) + [long_read(90, 100)])
    u = ar.concat_csr(res, bt, n_chroms=bt.n_chroms)
    out = []
    for c in ctxs:
        load(c, res)
        c.append_csr_any(bt, thr_of(bt))
        g = results(c, u)
        _, hits = c.search(u.iv_chrom[::3], u.iv_start[::3], u.iv_end[::3])
        out.append((repr(g), hits.tobytes(), repr(scores(c, u))))
    assert out[0] == out[1]


# ------------------------------------------------------------------ 7. the wrapper
def by_name(match_df):
    return sorted((min(a, b), max(a, b), j) for a, b, j in match_df.itertuples(index=False))


def clusters_of(G):
    return sorted(sorted(c) for c in cluster.get_subgraphs(G) if len(c) > 1)


def test_append_keeps_refusing_long_reads_and_append_any_takes_them():
    rng = np.random.default_rng(13)
    data = data_of(locus(60, rng), 1)
    long_d = mr.resident_data([long_read(70, 0)], [1000], [3])
    long_d.qnames = np.asarray(['long'], dtype=object)
    tree = cluster.build_interval_trees(data.select(np.asarray(data.qcode) < 40))
    with pytest.raises(NotImplementedError, match='append_any'):
        tree.append(long_d)
    assert tree.csr.n_reads == 40 and tree.long is None
    assert tree.append_any(long_d) is tree and tree.csr.n_reads == 41 and tree.long is not None
    with pytest.raises(NotImplementedError, match='append_any'):
        tree.append(data.select(np.asarray(data.qcode) >= 40))
    tree.append_any(data.select(np.asarray(data.qcode) >= 40))
    assert tree.csr.n_reads == 61 and len(tree.data) == len(data) + 70
    with pytest.raises(NotImplementedError, match='remove_any'):
        tree.remove(qnames=['long'])
    new_rank = tree.remove_any(qnames=['long'])
    assert new_rank[40] == -1 and tree.long is None and tree.csr.n_reads == 60
    tree.remove(keep=np.arange(60) % 2 == 0)                     # a plain index again
    assert tree.csr.n_reads == 30
    for cls in (cluster.RowsIndex, cluster.MultiGpuIndex):
        with pytest.raises(NotImplementedError, match='does not append'):
            cls.append_any(None, long_d)
        with pytest.raises(NotImplementedError, match='does not remove'):
            cls.remove_any(None, keep=[True])


def test_index_append_on_the_long_read_fixture_against_a_fresh_index():
    """longreads_400 split into resident + batch by qname: DeviceIntervalIndex.append against a fresh
    build_interval_trees of the union, in clusters, matches, search and match_reads_any."""
    data, _, kw = host_prepare('longreads_400')
    cut = [float(x) for x in kw['jaccard_cutoffs'].split(',')]
    args = (kw['overlap'], cut, 10, kw['qlen_diff'], kw['n_alignment_diff'])
    codes = np.unique(np.asarray(data.qcode))
    new_codes = np.random.default_rng(12).choice(codes, codes.size // 3, replace=False)
    is_new = np.isin(np.asarray(data.qcode), new_codes)
    res_d, new_d = data.select(~is_new), data.select(is_new)
    assert has_long_reads(res_d.csr()) and has_long_reads(new_d.csr())
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', cluster.EdgeCapWarning)
        tree = cluster.build_interval_trees(res_d)
        tree.append_any(new_d)
        assert tree.long is not None and tree.csr.n_reads == codes.size
        fresh = cluster.build_interval_trees(tree.data)
        m1, G1 = cluster.query_interval_trees(tree, tree.data, *args)
        m2, G2 = cluster.query_interval_trees(fresh, fresh.data, *args)
    assert len(m1) > 0 and by_name(m1) == by_name(m2)
    assert clusters_of(G1) == clusters_of(G2)
    k = np.arange(0, len(tree.data), 5)
    q = (tree.data.chrom[k], tree.data.start[k], tree.data.end[k])
    for x, y in zip(tree.search_batch(*q), fresh.search_batch(*q)):
        np.testing.assert_array_equal(x, y)
    r1 = tree.match_reads_any(new_d, kw['overlap'], cut, kw['qlen_diff'], kw['n_alignment_diff'])
    r2 = fresh.match_reads_any(new_d, kw['overlap'], cut, kw['qlen_diff'], kw['n_alignment_diff'])
    rows = lambda r: sorted(map(tuple, r.to_frame().itertuples(index=False)))     # by name: the two rank orders differ
    assert len(r1.partner) > 0 and rows(r1) == rows(r2)
    # ... and against the CPU oracle on the union's CSR (the edge cap applied as the reference applies it)
    o = O.run_core(oracle_from_csr(tree.csr), kw['overlap'], cut, kw['qlen_diff'], kw['n_alignment_diff'], 10)
    names = tree.data.qnames[np.asarray(tree.csr.read_qcode)]
    groups = {}
    for rank, comp in enumerate(o['comp'][:tree.csr.n_reads].tolist()):
        if comp >= 0:
            groups.setdefault(comp, []).append(names[rank])
    assert clusters_of(G1) == sorted(sorted(g) for g in groups.values())
