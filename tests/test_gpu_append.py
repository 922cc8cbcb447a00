"""fslr_append_reads / DeviceIntervalIndex.append: reads added to a resident set on the device.

The yardstick of every equality case is a FRESH context given fslr_set_reads of the concatenated CSR with the
reference-merged iv_data_pos (append_ref.concat_csr).  After build_index + query on both contexts the edges
(a, b, I, U), the forward degrees, the labels, fslr_read_stats' counts and the hits of a search batch (in
order: the search order ranks ties by data position, so it shows the merged data order) are compared
exactly.  The last case compares with the CPU oracle and a golden fixture's expected clusters instead.
"""
import ctypes
import dataclasses
import hashlib
import warnings

import numpy as np
import pytest

import append_ref as ar
import fixtures as fx
import match_ref as mr
from host_pipeline import host_prepare
from fslr_amd import _lib, cluster, synth
from fslr_amd._lib import APPEND_TILE, FSLR_ERR_INVALID, FSLR_ERR_STATE, FSLR_THR_ZERO_ALN
from fslr_amd.prep import fold_overlap_threshold, pass_table
from oracle import oracle as O
from test_gpu_parity import oracle_from_csr

pytestmark = pytest.mark.gpu

CUTOFFS = (1, 1, 0.66, 0.66, 0.66, 0.5)
PCT, QD, ND = 0.8, 0.04, 0.25
PT = pass_table(CUTOFFS)
# (err_a / err_b are left out: which of several raising pairs a query names depends on its schedule)
COUNTS = ('n_edges', 'max_fwd', 'candidates', 'evaluated_pairs', 'jaccard_evals', 'match_entries', 'matched_pairs',
          'pair_tests', 'zd_pairs', 'engine', 'error')


@pytest.fixture
def ctxs():
    """Two contexts of their own for every test (a shared context's buffers only grow): the one that appends
    and the fresh yardstick."""
    a, b = _lib.Context(0), _lib.Context(0)
    yield a, b
    a.close()
    b.close()


def thr_of(csr, pct=PCT):
    return fold_overlap_threshold(csr.iv_aln, pct)


def rebased(res_data, res_csr, new_data):
    """The new rows' CSR with its chromosomes in the resident dense ids (unseen values behind them, ascending)."""
    nc = new_data.csr()
    keys, first = np.unique(np.asarray(res_data.chrom)[res_csr.data_pos], return_index=True)
    lut = dict(zip(keys.tolist(), res_csr.iv_chrom[first].tolist()))
    raw = np.asarray(new_data.chrom)[nc.data_pos]
    unseen = np.setdiff1d(raw, keys)
    lut.update({v: res_csr.n_chroms + k for k, v in enumerate(unseen.tolist())})
    return dataclasses.replace(nc, iv_chrom=np.asarray([lut[v] for v in raw.tolist()], np.int32),
                               n_chroms=int(res_csr.n_chroms + unseen.size))


def split(data, new_codes):
    """(resident rows, new rows) of a data list by qname code."""
    is_new = np.isin(np.asarray(data.qcode), new_codes)
    return data.select(~is_new), data.select(is_new)


def raw_stats(ctx):
    """fslr_read_stats' struct whatever its return code (a ZeroDivisionError report is a result here)."""
    s = _lib.QueryStats()
    ctx._L.fslr_read_stats(ctx._h, ctypes.byref(s))
    return s.as_dict()


def graph(ctx, n_reads, engine='auto', cap=None, edge_threshold=10):
    """build_index + query (+ the edge cap) + components; what the cases compare."""
    ctx.reserve_edges(max(1 << 16, 12 * n_reads))
    ctx.build_index()
    out = {'raised': False}
    try:
        st = ctx.run_query(1 - QD, 1 - ND, PT, edge_threshold, engine=engine)
    except ZeroDivisionError:
        st = raw_stats(ctx)
        out['raised'] = True
    if cap is not None:
        out['cap'] = ctx.apply_edge_cap(cap)
    a, b, I, U = ctx.edges(raw_stats(ctx)['n_edges'])
    out.update(edges=sorted(zip(a.tolist(), b.tolist(), I.tolist(), U.tolist())), fwd=ctx.fwd_degree(),
               counts={k: st[k] for k in COUNTS})
    if not out['raised']:                                   # the reference has no graph after a raise
        ctx.components()
        out['labels'] = ctx.labels()
    return out


def same_graph(got, want, what=''):
    assert got['counts'] == want['counts'], what
    assert got.get('raised') == want.get('raised') and got.get('cap') == want.get('cap'), what
    assert got['edges'] == want['edges'], what
    np.testing.assert_array_equal(got['fwd'], want['fwd'], err_msg=what)
    np.testing.assert_array_equal(got.get('labels'), want.get('labels'), err_msg=what)


def same_search(ca, cb, u, what='', limit=4000):
    """Every interval of the union (or an even sample) as a query: the same hits in the same order."""
    k = np.unique(np.linspace(0, u.n_intervals - 1, min(limit, u.n_intervals)).astype(np.int64))
    q = (u.iv_chrom[k], u.iv_start[k], u.iv_end[k])
    (oa, ha), (ob, hb) = ca.search(*q), cb.search(*q)
    np.testing.assert_array_equal(oa, ob, err_msg=what)
    np.testing.assert_array_equal(ha, hb, err_msg=what)
    return oa, ha


def append_vs_fresh(ctxs, res, batches, engine='auto', cap=None, pcts=None, built=True, what=''):
    """Resident CSR ``res`` plus the batches (rebased CSRs), appended one after the other, against one fresh
    upload of the iteratively concatenated CSR.  Returns (appended graph, union CSR)."""
    ca, cb = ctxs
    pcts = pcts or [PCT] * (len(batches) + 1)
    ca.load_csr(res, thr_of(res, pcts[0]))
    if built:
        ca.build_index()
    u, thr = res, thr_of(res, pcts[0])
    for bt, pct in zip(batches, pcts[1:]):
        ca.append_csr(bt, thr_of(bt, pct))
        u = ar.concat_csr(u, bt, n_chroms=bt.n_chroms)
        thr = np.concatenate([thr, thr_of(bt, pct)])
    assert ca.n_reads == u.n_reads and ca.n_intervals == u.n_intervals
    cb.load_csr(u, thr)
    g, w = graph(ca, u.n_reads, engine, cap), graph(cb, u.n_reads, engine, cap)
    same_graph(g, w, what)
    same_search(ca, cb, u, what)
    return g, u


def synth_split(n_res, n_new, seed=3, lmax=8):
    data = synth.generate(n_res + n_new, lmax, seed).interval_data()
    codes = np.unique(np.asarray(data.qcode))
    new_codes = np.random.default_rng(seed).choice(codes, n_new, replace=False)
    return data, new_codes


# ------------------------------------------------------------------ 1. basic
@pytest.mark.parametrize('engine', ['walk', 'sweep'])
def test_basic_split_by_read(ctxs, engine):
    data, new_codes = synth_split(2000, 300)
    res_d, new_d = split(data, new_codes)
    res = res_d.csr()
    g, u = append_vs_fresh(ctxs, res, [rebased(res_d, res, new_d)], engine=engine)
    assert g['counts']['engine'] == engine and g['counts']['n_edges'] > 500
    new_rank = np.arange(res.n_reads, u.n_reads)
    assert any(a < res.n_reads <= b for a, b, _, _ in g['edges'])          # edges between old and new reads
    assert np.isin(g['labels'][new_rank], np.arange(res.n_reads)).any()


def test_three_batches_against_one_fresh_upload(ctxs):
    data, new_codes = synth_split(2000, 300)
    res_d, _ = split(data, new_codes)
    res = res_d.csr()
    batches = [rebased(res_d, res, split(data, new_codes[k:k + 100])[1]) for k in (0, 100, 200)]
    _, u = append_vs_fresh(ctxs, res, batches)
    assert u.n_reads == res.n_reads + 300


# ------------------------------------------------------------------ 2. ties
def one_locus(n_reads, starts, rng, chrom=1):
    """Single- and two-interval reads on one chromosome with the given pool of starts."""
    reads = []
    for _ in range(n_reads):
        L = int(rng.integers(1, 3))
        reads.append([(chrom, int(s), int(s) + 100, 100) for s in np.sort(rng.choice(starts, L))])
    return reads


def lists_case(res_reads, *new_lists, seeds=(1, 2)):
    """(resident CSR, rebased batch CSR, ...) of read lists (match_ref.resident_data, shuffled ties)."""
    res_d = mr.resident_data(res_reads, np.full(len(res_reads), 1000), np.full(len(res_reads), 3), shuffle_seed=seeds[0])
    res = res_d.csr()
    out = [res]
    for t, reads in enumerate(new_lists):
        d = mr.resident_data(reads, np.full(len(reads), 1000), np.full(len(reads), 3), shuffle_seed=seeds[1] + t)
        out.append(rebased(res_d, res, d))
    return tuple(out)


def test_eight_start_values(ctxs):
    """All starts from 8 values: long equal-start runs cross between resident and new.  The search order
    (ties ranked by data position) shows the resident-first rule; the cap-binding query replays it."""
    rng = np.random.default_rng(8)
    starts = np.arange(8) * 10
    res, bt = lists_case(one_locus(200, starts, rng), one_locus(80, starts, rng))
    g, u = append_vs_fresh(ctxs, res, [bt], cap=3)
    assert g['cap']['applied'] == 1 and g['cap']['capped'] > 0
    # resident first inside every run of equal (start, end): hits come in descending data position
    ca = ctxs[0]
    off, hits = ca.search(np.zeros(1, np.int32), np.zeros(1, np.int32), np.full(1, 1000, np.int32))
    assert hits.size == u.n_intervals
    s = u.iv_start[hits]
    run = np.flatnonzero(np.diff(s) == 0)
    is_new = hits >= res.n_intervals
    assert run.size > 100 and not (~is_new[run] & is_new[run + 1]).any()     # descending: new before resident


def seam_lists(total, lo, hi, rng):
    """Single-interval reads whose merged list has ``total`` elements, with one run of equal starts over the
    merged positions [lo, hi) and distinct starts elsewhere; each element resident or new at random."""
    s = 4 * np.arange(total, dtype=np.int64)
    s[lo:min(hi, total)] = s[lo]
    is_new = rng.random(total) < 0.3
    is_new[lo], is_new[min(hi, total) - 1] = False, True            # the run holds both kinds
    mk = lambda v: [[(1, int(x), int(x) + 6, 6)] for x in v]
    return mk(s[~is_new]), mk(s[is_new])


def test_tie_runs_across_the_merge_tile_seams(ctxs):
    """k_append_merge cuts its output into tiles of T = FSLR_APPEND_TILE elements: merged lengths and tie
    runs that end and begin at T - 1, T and T + 1 (and the same around 2 T)."""
    T = APPEND_TILE
    assert T == 1024
    rng = np.random.default_rng(10)
    for base in (T, 2 * T):
        for total in (base - 1, base, base + 1):
            for lo, hi in ((base - 7, base - 1), (base - 7, base), (base - 7, base + 1), (base - 1, base + 6),
                           (base, base + 6), (base + 1, base + 6)):
                if lo >= total - 1:
                    continue
                res, bt = lists_case(*seam_lists(total, lo, hi, rng), seeds=(total, lo + hi))
                assert res.n_intervals + bt.n_intervals == total
                append_vs_fresh(ctxs, res, [bt], what=f'total {total} run [{lo}, {hi})')


# ------------------------------------------------------------------ 3. the cap binding
def test_cap_binds_on_a_shared_locus(ctxs):
    """One locus shared by 60 resident and 30 new reads, edge_threshold 3."""
    rng = np.random.default_rng(3)
    mk = lambda n: [[(2, 500 + int(rng.integers(0, 5)), 700, 200)] for _ in range(n)]
    res, bt = lists_case(mk(60), mk(30))
    g, _ = append_vs_fresh(ctxs, res, [bt], cap=3)
    assert g['cap']['applied'] == 1 and g['counts']['max_fwd'] > 3 and g['cap']['dropped'] > 0


# ------------------------------------------------------------------ 4. placement
@pytest.mark.parametrize('where', ['below', 'above', 'one'])
def test_placement(ctxs, where):
    """3000 resident intervals (three merge tiles) with the batch below all of them, above all of them, and a
    batch of one read in the middle: tiles of one list alone are straight copies."""
    res_reads = [[(1, 100_000 + 4 * k, 100_000 + 4 * k + 25, 25)] for k in range(3000)]
    base = {'below': 0, 'above': 200_000, 'one': 106_001}[where]
    new_reads = [[(1, base + 4 * k, base + 4 * k + 25, 25)] for k in range(1 if where == 'one' else 700)]
    res, bt = lists_case(res_reads, new_reads)
    g, u = append_vs_fresh(ctxs, res, [bt], what=where)
    if where == 'one':
        assert any(b == u.n_reads - 1 for _, b, _, _ in g['edges'])


def test_empty_batch_is_a_no_op(ctxs):
    ca, _ = ctxs
    data, _ = synth_split(500, 0)
    csr = data.csr()
    ca.load_csr(csr, thr_of(csr))
    want = graph(ca, csr.n_reads)
    off, hits = ca.search(csr.iv_chrom[:50], csr.iv_start[:50], csr.iv_end[:50])
    z = np.zeros(0, np.int32)
    ca.append_reads(np.zeros(1, np.int32), z, z, z, z, z, z, csr.n_chroms, z)
    assert ca.n_reads == csr.n_reads
    again = np.empty(hits.size, np.int32)                     # the saved batch still reads: no generation moved
    assert ca._L.fslr_search_hits(ca._h, again.ctypes.data_as(ctypes.c_void_p), hits.size) == 0
    np.testing.assert_array_equal(again, hits)
    st = ca.run_query(1 - QD, 1 - ND, PT)                     # and the index is still built
    assert st['n_edges'] == want['counts']['n_edges']


# ------------------------------------------------------------------ 5. growth
def test_buffers_grow_with_their_contents(ctxs):
    """3 resident reads, 5000 appended (every buffer grows), then 3 more (nothing grows)."""
    rng = np.random.default_rng(12)
    pool = np.arange(20_000) * 40
    res_reads = [[(c, 400_000, 400_100, 100)] for c in (1, 2, 3)]
    many = [r for c in (1, 2, 3) for r in one_locus(1667, pool, rng, chrom=c)][:5000]
    more = [[(c, 400_010, 400_110, 100)] for c in (1, 2, 3)]
    res, b1, b2 = lists_case(res_reads, many, more)
    assert res.n_reads == 3 and b1.n_reads == 5000 and b1.n_chroms == b2.n_chroms == 3
    g, u = append_vs_fresh(ctxs, res, [b1, b2])
    assert u.n_reads == 5006 and sum(1 for a, b, _, _ in g['edges'] if a < 3 and b >= 5003) == 3


# ------------------------------------------------------------------ 6. chromosomes
def test_new_chromosome_id(ctxs):
    rng = np.random.default_rng(6)
    res_reads = one_locus(300, np.arange(40) * 7, rng, chrom=1) + one_locus(300, np.arange(40) * 7, rng, chrom=2)
    new_reads = one_locus(50, np.arange(40) * 7, rng, chrom=2) + one_locus(50, np.arange(40) * 7, rng, chrom=9)
    res, bt = lists_case(res_reads, new_reads)
    assert bt.n_chroms == res.n_chroms + 1 == 3 and (bt.iv_chrom == 2).any()
    g, u = append_vs_fresh(ctxs, res, [bt])
    on_new = np.flatnonzero(u.iv_chrom == 2)
    assert len(g['edges']) > 100 and on_new.size >= 50


def test_sixty_fifth_chromosome(ctxs):
    """64 resident chromosomes (the counting-sort limit of the index build) plus a read on the 65th: the
    rebuilt index takes the radix fallback."""
    rng = np.random.default_rng(65)
    res_reads = [r for c in range(1, 65) for r in one_locus(12, np.arange(6) * 9, rng, chrom=c)]
    new_reads = one_locus(12, np.arange(6) * 9, rng, chrom=65) + one_locus(12, np.arange(6) * 9, rng, chrom=64)
    res, bt = lists_case(res_reads, new_reads)
    assert res.n_chroms == 64 and bt.n_chroms == 65
    g, _ = append_vs_fresh(ctxs, res, [bt])
    assert len(g['edges']) > 500


# ------------------------------------------------------------------ 7. threshold modes
def test_batch_brings_a_zero_aln_interval(ctxs):
    rng = np.random.default_rng(7)
    res_reads = one_locus(300, np.arange(30) * 5, rng)
    new_reads = one_locus(60, np.arange(30) * 5, rng)
    c, s, e, _ = new_reads[7][0]
    new_reads[7][0] = (c, s, e, 0)
    res, bt = lists_case(res_reads, new_reads)
    assert (thr_of(bt) == FSLR_THR_ZERO_ALN).sum() == 1 and not (thr_of(res) == FSLR_THR_ZERO_ALN).any()
    g, _ = append_vs_fresh(ctxs, res, [bt])
    assert g['counts']['engine'] == 'walk' and (g['raised'] or g['counts']['zd_pairs'] > 0)


def test_batch_brings_a_threshold_below_one(ctxs):
    rng = np.random.default_rng(17)
    res, bt = lists_case(one_locus(300, np.arange(30) * 5, rng), one_locus(60, np.arange(30) * 5, rng))
    g, _ = append_vs_fresh(ctxs, res, [bt], pcts=[PCT, 0.0])
    assert (thr_of(bt, 0.0) < 1).all() and g['counts']['engine'] == 'walk' and len(g['edges']) > 100


# ------------------------------------------------------------------ 8. after use
def table_answer(c):
    """fslr_get_cluster_ids' answer: the resident table's (cid, size), or 'refused'."""
    try:
        return [x.tolist() for x in c.cluster_ids()]
    except _lib.FslrError:
        return 'refused'


def test_append_after_the_context_was_used(ctxs):
    """A context that has run a sweep query on the lean index, a search, a match and a cluster table."""
    ca, cb = ctxs
    data, new_codes = synth_split(1500, 200, seed=21)
    res_d, new_d = split(data, new_codes)
    res = res_d.csr()
    bt = rebased(res_d, res, new_d)
    ca.load_csr(res, thr_of(res))
    g0 = graph(ca, res.n_reads, 'sweep')
    assert g0['counts']['engine'] == 'sweep'
    ca.cluster_table()
    table0 = table_answer(ca)
    assert table0 != 'refused' and max(table0[1]) >= 2
    _, hits = ca.search(res.iv_chrom[:64], res.iv_start[:64], res.iv_end[:64])
    q = (bt.read_off[:11], bt.read_qlen2[:10], bt.read_nal[:10], bt.iv_chrom[:bt.read_off[10]],
         bt.iv_start[:bt.read_off[10]], bt.iv_end[:bt.read_off[10]], thr_of(bt)[:bt.read_off[10]])
    ca.match_reads(*q, 1 - QD, 1 - ND, PT)
    ca.match_rows()
    ca.append_csr(bt, thr_of(bt))
    buf = np.empty(max(hits.size, 1), np.int32)
    assert ca._L.fslr_search_hits(ca._h, buf.ctypes.data_as(ctypes.c_void_p), buf.size) == FSLR_ERR_STATE
    with pytest.raises(_lib.FslrError, match='error 5'):
        ca.match_rows()
    u = ar.concat_csr(res, bt, n_chroms=bt.n_chroms)
    # the old cluster table answers what it answers after fslr_set_reads: the yardstick context makes the
    # same table on the resident reads before it takes the union.  (The library keeps no score batch:
    # fslr_score_pairs returns its results in the call; it is asked again below.)
    cb.load_csr(res, thr_of(res))
    same_graph(graph(cb, res.n_reads, 'sweep'), g0)
    cb.cluster_table()
    cb.load_csr(u, np.concatenate([thr_of(res), thr_of(bt)]))
    assert table_answer(ca) == table_answer(cb) and table_answer(ca) == table0
    g, w = graph(ca, u.n_reads, 'sweep'), graph(cb, u.n_reads, 'sweep')
    same_graph(g, w)
    same_search(ca, cb, u)
    mixed = [(a, b) for a, b, _, _ in g['edges'] if a < res.n_reads <= b][:50]
    assert len(mixed) > 10
    pa, pb = np.array(mixed, np.int32).T
    for x, y in zip(ca.score_pairs(pa, pb, 1 - QD, 1 - ND, PT), cb.score_pairs(pa, pb, 1 - QD, 1 - ND, PT)):
        np.testing.assert_array_equal(x, y)
    assert (ca.score_pairs(pa, pb, 1 - QD, 1 - ND, PT)[2] & _lib.SCORE_EDGE).all()
    ex = np.arange(res.n_reads, res.n_reads + 10, dtype=np.int32)        # ask about resident (new-rank) reads
    ma, mb = ca.match_reads(*q, 1 - QD, 1 - ND, PT, exclude=ex), cb.match_reads(*q, 1 - QD, 1 - ND, PT, exclude=ex)
    for x, y in zip(ma + ca.match_rows(), mb + cb.match_rows()):
        np.testing.assert_array_equal(x, y)


# ------------------------------------------------------------------ 9. refusals and atomicity
def raw_append(ctx, csr, thr, **over):
    """fslr_append_reads with fields of the batch replaced; returns (rc, message)."""
    f = dict(read_off=csr.read_off, read_qlen2=csr.read_qlen2, read_nal=csr.read_nal, iv_chrom=csr.iv_chrom,
             iv_start=csr.iv_start, iv_end=csr.iv_end, iv_thr=thr, iv_data_pos=csr.data_pos, n_chroms=csr.n_chroms)
    f.update(over)
    n_chroms = int(f.pop('n_chroms'))
    arrs = {k: None if v is None else np.ascontiguousarray(v, np.int32) for k, v in f.items()}
    p = lambda k: None if arrs[k] is None else arrs[k].ctypes.data_as(ctypes.c_void_p)
    r = _lib.Reads(len(arrs['read_qlen2']), len(arrs['iv_start']), n_chroms,
                   *(p(k) for k in ('read_off', 'read_qlen2', 'read_nal', 'iv_chrom', 'iv_start', 'iv_end', 'iv_thr',
                                    'iv_data_pos')))
    rc = ctx._L.fslr_append_reads(ctx._h, ctypes.byref(r))
    return rc, (ctx._L.fslr_last_error(ctx._h) or b'').decode()


def test_invalid_batches_leave_the_context_untouched(ctxs):
    ca, _ = ctxs
    rng = np.random.default_rng(9)
    res, bt = lists_case(one_locus(400, np.arange(50) * 6, rng), one_locus(40, np.arange(50) * 6, rng))
    thr = thr_of(bt)
    ca.load_csr(res, thr_of(res))
    want = graph(ca, res.n_reads)
    q = (res.iv_chrom[:40], res.iv_start[:40], res.iv_end[:40])
    _, hits = ca.search(*q)
    rep = lambda a, k, v: np.concatenate([a[:k], [v], a[k + 1:]])
    long_off = np.concatenate([[0], np.full(bt.n_reads, 65)]).cumsum()
    swapped = bt.data_pos.copy()
    lo, hi = np.argmin(bt.iv_start), np.argmax(bt.iv_start)
    swapped[[lo, hi]] = swapped[[hi, lo]]
    zero_off = bt.read_off.copy()
    zero_off[1] = 0                                                 # read 0 without an interval
    bad = [
        (dict(iv_chrom=rep(bt.iv_chrom, 3, bt.n_chroms)), 'chrom id out of range'),
        (dict(iv_chrom=rep(bt.iv_chrom, 3, -1)), 'chrom id out of range'),
        (dict(iv_end=rep(bt.iv_end, 5, 1 << 30)), 'interval coordinates out of [0, 2^30)'),
        (dict(read_off=zero_off), 'every read needs 1..64 intervals'),
        (dict(read_off=long_off, **{k: np.resize(getattr(bt, k), 65 * bt.n_reads) for k in
                                    ('iv_chrom', 'iv_start', 'iv_end')}, iv_thr=np.resize(thr, 65 * bt.n_reads),
              iv_data_pos=np.arange(65 * bt.n_reads)), 'every read needs 1..64 intervals'),
        (dict(read_nal=rep(bt.read_nal, 2, 1 << 24)), 'n_alignments outside [0, 2^24)'),
        (dict(read_qlen2=rep(bt.read_qlen2, 2, -1)), 'qlen2 < 0'),
        (dict(iv_data_pos=swapped), 'iv_data_pos is not a start-sorted permutation'),
        (dict(iv_data_pos=rep(bt.data_pos, 0, bt.data_pos[1])), 'iv_data_pos is not a start-sorted permutation'),
        (dict(iv_data_pos=None), 'iv_data_pos is required'),
        (dict(n_chroms=0), 'n_chroms out of range'),
    ]
    for over, msg in bad:
        rc, text = raw_append(ca, bt, thr, **over)
        assert rc == FSLR_ERR_INVALID, (over.keys(), rc, text)
        assert msg is None or msg in text, (over.keys(), text)
        assert ca.n_reads == res.n_reads
        again = np.empty(hits.size, np.int32)                       # the earlier search batch still reads
        assert ca._L.fslr_search_hits(ca._h, again.ctypes.data_as(ctypes.c_void_p), hits.size) == 0, over.keys()
        np.testing.assert_array_equal(again, hits)
        st = ca.run_query(1 - QD, 1 - ND, PT)                       # no rebuild: the index is still built
        a, b, I, U = ca.edges(st['n_edges'])
        assert sorted(zip(a.tolist(), b.tolist(), I.tolist(), U.tolist())) == want['edges'], over.keys()
    rc, text = raw_append(ca, bt, thr)                              # and the good batch still goes in
    assert rc == 0, text


def test_n_chroms_below_the_resident_value(ctxs):
    ca, _ = ctxs
    rng = np.random.default_rng(19)
    res, bt = lists_case(one_locus(50, np.arange(9), rng, 1) + one_locus(50, np.arange(9), rng, 2), one_locus(5, np.arange(9), rng, 1))
    ca.load_csr(res, thr_of(res))
    rc, text = raw_append(ca, bt, thr_of(bt), n_chroms=1)
    assert rc == FSLR_ERR_INVALID and 'n_chroms below the resident value' in text


def test_state_refusals(ctxs):
    ca, _ = ctxs
    rng = np.random.default_rng(29)
    res, bt = lists_case(one_locus(100, np.arange(20) * 3, rng), one_locus(10, np.arange(20) * 3, rng))
    thr = thr_of(bt)

    def refused(word):
        rc, text = raw_append(ca, bt, thr)
        assert rc == FSLR_ERR_STATE and word in text, (word, rc, text)
    refused('no reads set')
    ca.set_reads(res.read_off, res.read_qlen2, res.read_nal, res.iv_chrom, res.iv_start, res.iv_end, thr_of(res), res.n_chroms)
    refused('without iv_data_pos')
    long_reads = [[(1, 10 * k, 10 * k + 50, 50) for k in range(70)]] + one_locus(5, np.arange(20) * 3, rng)
    lc = mr.resident_data(long_reads, np.full(6, 1000), np.full(6, 3)).csr()
    ca.load_csr_any(lc, thr_of(lc))
    refused('virtual reads')
    ca.load_csr(res, thr_of(res))
    ca.set_shard(0, 2)
    refused('n_shards > 1')
    ca.set_shard(0, 1)
    ca.set_chrom_filter(np.ones(res.n_chroms, bool))
    refused('filter')
    ca.set_chrom_filter(None)
    ca.build_index()
    ca.set_position_filter(0, res.n_intervals, res.n_intervals)      # a position filter over every position
    refused('filter')
    ca.load_csr(res, thr_of(res))                                    # (an upload drops the filter)
    n = 6
    cols = dict(chrom=np.ones(n), start=np.arange(n) * 5, end=np.arange(n) * 5 + 40, aln=np.full(n, 40),
                qcode=np.arange(n) // 2, nal=np.full(n, 3), qlen2=np.full(n, 1000))
    ca.rows_upload(cols, 3, 2)
    ca.set_reads_rows(np.arange(n), None, PCT)
    refused('rows')
    ca.load_csr(res, thr_of(res))                                    # and a plain context appends again
    rc, text = raw_append(ca, bt, thr)
    assert rc == 0, text


def test_python_refusals():
    rng = np.random.default_rng(39)
    reads = one_locus(60, np.arange(20) * 3, rng)
    data = mr.resident_data(reads, np.full(60, 1000), np.full(60, 3), shuffle_seed=1)
    tree = cluster.build_interval_trees(data.select(np.asarray(data.qcode) < 40))
    with pytest.raises(ValueError, match='already a read of this index'):
        tree.append(data.select(np.isin(data.qcode, [39, 45])))
    long_d = mr.resident_data([[(1, 10 * k, 10 * k + 50, 50) for k in range(70)]], [1000], [3])
    long_d.qnames = np.asarray(['long'], dtype=object)
    with pytest.raises(NotImplementedError, match='more than 64 intervals'):
        tree.append(long_d)
    assert tree.csr.n_reads == 40
    tree.append(data.select(np.asarray(data.qcode) >= 40))
    assert tree.csr.n_reads == 60 and len(tree.data) == len(data)
    long_tree = cluster.build_interval_trees(long_d)
    with pytest.raises(NotImplementedError, match='more than 64 intervals'):
        long_tree.append(data)


def test_wrapper_thresholds_survive_an_append():
    """score_pairs and match_reads skip fslr_set_thresholds while the overlap they last folded is installed.
    An append in between must leave the new reads' thresholds folded for that overlap too: r1 (new, aln_size
    100) shares 60 with r0 (old, aln_size 50) and with the query read (aln_size 50), which is 1.2 of their
    size but only 0.6 of r1's: below the 0.8 asked for, above a threshold of 0."""
    import pandas as pd
    reads = [[(1, 1000, 1100, 50)], [(1, 1040, 1140, 100)], [(1, 1080, 1180, 50)], [(1, 5000, 5100, 100)]]
    data = mr.resident_data(reads, np.full(4, 1000), np.full(4, 3))
    code = np.asarray(data.qcode)
    args = (PCT, list(CUTOFFS), QD, ND)
    tree = cluster.build_interval_trees(data.select(np.isin(code, [0, 3])))
    query = data.select(code == 2)
    before = tree.match_reads(query, *args, emit='all').to_frame()
    tree.score_pairs(['r0'], ['r3'], *args)
    tree.append(data.select(code == 1))
    fresh = cluster.build_interval_trees(tree.data)
    got, want = tree.match_reads(query, *args, emit='all'), fresh.match_reads(query, *args, emit='all')
    pd.testing.assert_frame_equal(got.to_frame(), want.to_frame())
    assert len(got.to_frame()) == len(before) + 1 and not (got.flags & _lib.SCORE_EDGE).any() and (got.I == 0).all()
    for a, b in (('r0', 'r1'), ('r1', 'r0'), ('r1', 'r1')):
        s, w = tree.score_pairs([a], [b], *args), fresh.score_pairs([a], [b], *args)
        assert (s.I.tolist(), s.U.tolist(), s.flags.tolist()) == (w.I.tolist(), w.U.tolist(), w.flags.tolist()), (a, b)
        assert (s.I[0] == 1) == (a == b), (a, b)


# ------------------------------------------------------------------ 10. determinism
def test_two_appends_give_the_same_bytes(ctxs):
    ca, cb = ctxs
    data, new_codes = synth_split(2000, 300, seed=31)
    res_d, new_d = split(data, new_codes)
    res = res_d.csr()
    bt = rebased(res_d, res, new_d)
    out = []
    for c in (ca, cb):
        c.load_csr(res, thr_of(res))
        c.build_index()
        c.append_csr(bt, thr_of(bt))
        g = graph(c, res.n_reads + bt.n_reads)
        out.append((hashlib.sha256(repr(g['edges']).encode()).hexdigest(), g['labels'].tobytes(), g['fwd'].tobytes()))
    assert out[0] == out[1]
    same_search(ca, cb, ar.concat_csr(res, bt, n_chroms=bt.n_chroms))


# ------------------------------------------------------------------ DeviceIntervalIndex.append
def by_name(match_df):
    return sorted((min(a, b), max(a, b), j) for a, b, j in match_df.itertuples(index=False))


def test_index_append_against_a_fresh_index():
    """build_interval_trees on the resident rows + append of the new rows against build_interval_trees of the
    merged list (tree.data): the same match set and clusters by qname, the same hits by data position."""
    data, new_codes = synth_split(2000, 300, seed=41)
    res_d, new_d = split(data, new_codes)
    args = (PCT, list(CUTOFFS), 10, QD, ND)
    tree = cluster.build_interval_trees(res_d).append(new_d)
    assert tree.source is tree.data and len(tree.data) == len(data)
    np.testing.assert_array_equal(tree.data.start, np.sort(data.start))
    m1, G1 = cluster.query_interval_trees(tree, tree.data, *args)
    fresh = cluster.build_interval_trees(tree.data)
    m2, G2 = cluster.query_interval_trees(fresh, tree.data, *args)
    assert len(m1) > 500 and by_name(m1) == by_name(m2)
    assert sorted(sorted(c) for c in cluster.get_subgraphs(G1)) == sorted(sorted(c) for c in cluster.get_subgraphs(G2))
    k = np.arange(0, len(data), 7)
    q = (tree.data.chrom[k], tree.data.start[k], tree.data.end[k])
    for x, y in zip(tree.search_batch(*q), fresh.search_batch(*q)):
        np.testing.assert_array_equal(x, y)


# ------------------------------------------------------------------ 11. the reference's semantics
def test_golden_fixture_built_in_two_halves():
    """mixed_2k_l8 (2000 reads, 8774 intervals; the oracle's max forward degree on it is 9 <= 10, so the edge
    cap does not bind; no aln_size == 0 interval, n_alignments constant inside every read), split by qname into
    two halves: one built, the other appended.  The clusters as sets of qnames equal the fixture's expected
    components and the edges as unordered name pairs with (I, U) equal the oracle's on the whole input.  A
    pair's (I, U) does not depend on which read is list1 (first-fit's symmetry): the two rank
    numberings may orient a pair differently; a fixture pair that violated it would be named below."""
    name = 'mixed_2k_l8'
    data, _, kw = host_prepare(name)
    cut = [float(x) for x in kw['jaccard_cutoffs'].split(',')]
    whole = data.csr()
    assert not whole.nal_varies and not (whole.iv_aln == 0).any()
    o = O.run_core(oracle_from_csr(whole), kw['overlap'], cut, kw['qlen_diff'], kw['n_alignment_diff'], 10, use_cap=False)
    assert o['stats']['max_fwd'] == 9
    names = np.asarray(data.qnames)[whole.read_qcode]
    want = {(min(x, y), max(x, y)): (i, u) for x, y, i, u in
            zip(names[o['edge_a']].tolist(), names[o['edge_b']].tolist(), o['edge_I'].tolist(), o['edge_U'].tolist())}
    codes = np.unique(np.asarray(data.qcode))
    second = np.isin(np.asarray(data.qcode), codes[codes.size // 2:])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', cluster.EdgeCapWarning)
        tree = cluster.build_interval_trees(data.select(~second)).append(data.select(second))
        g = cluster.query_graph(tree, tree.data, kw['overlap'], cut, 10, kw['qlen_diff'], kw['n_alignment_diff'])
        ga, gb, gI, gU = (np.array(x) for x in (g.a, g.b, g.I, g.U))          # fetched before the next query
        _, G = cluster.query_interval_trees(tree, tree.data, kw['overlap'], cut, 10, kw['qlen_diff'], kw['n_alignment_diff'])
    gn = np.asarray(tree.data.qnames)[tree.csr.read_qcode]
    got = {(min(x, y), max(x, y)): (i, u) for x, y, i, u in
           zip(gn[ga].tolist(), gn[gb].tolist(), gI.tolist(), gU.tolist())}
    differ = [(p, got.get(p), want.get(p)) for p in sorted(set(got) | set(want)) if got.get(p) != want.get(p)]
    assert not differ, f'{len(differ)} pairs differ, the first: {differ[0]}'
    assert len(got) == 3463
    assert sorted(sorted(c) for c in cluster.get_subgraphs(G)) == sorted(sorted(c) for c in fx.stage(name)['components'])
