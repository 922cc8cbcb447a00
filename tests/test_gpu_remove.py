"""fslr_remove_reads / DeviceIntervalIndex.remove: whole reads dropped from a resident set on the device.

The yardstick of every equality case is a FRESH context given fslr_set_reads of remove_ref.remove_csr(csr, keep)
with the survivors' thresholds.  After build_index + query on both contexts the edges (a, b, I, U), the forward
degrees, the labels, fslr_read_stats' counts and the hits of a search batch (in order: the search order ranks
ties by data position, so it shows the compacted data order) are compared exactly (test_gpu_append's graph()
and same_search()).  The small cases come first.
"""
import ctypes
import warnings

import numpy as np
import pytest

import append_ref as ar
import match_ref as mr
import remove_ref as rr
from host_pipeline import host_prepare
from fslr_amd import _lib, cluster, synth
from fslr_amd._lib import FSLR_ERR_INVALID, FSLR_ERR_STATE, FSLR_THR_ZERO_ALN, REMOVE_TILE
from oracle import oracle as O
from test_gpu_append import (CUTOFFS, ND, PCT, PT, QD, graph, lists_case, one_locus, rebased, same_graph, same_search,
                             split, synth_split, thr_of)
from test_gpu_parity import oracle_from_csr

pytestmark = pytest.mark.gpu

T = REMOVE_TILE


@pytest.fixture
def ctxs():
    """Two contexts of their own for every test: the one that removes and the fresh yardstick."""
    a, b = _lib.Context(0), _lib.Context(0)
    yield a, b
    a.close()
    b.close()


def kept_iv(csr, keep):
    """Per CSR interval: does its read stay."""
    return np.repeat(np.asarray(keep, bool), np.diff(np.asarray(csr.read_off, np.int64)))


def remove_vs_fresh(ctxs, csr, keeps, thr=None, engine='auto', cap=None, built=True, what=''):
    """The CSR uploaded and the masks applied one after the other (each over the ranks the one before left),
    against one fresh upload of the iterated remove_ref.remove_csr.  Returns (graph, compacted CSR)."""
    ca, cb = ctxs
    thr = thr_of(csr) if thr is None else thr
    ca.load_csr(csr, thr)
    if built:
        ca.build_index()
    for keep in keeps:
        got = ca.remove_reads(keep)
        np.testing.assert_array_equal(got, rr.rank_map(keep), err_msg=what)
        thr = thr[kept_iv(csr, keep)]
        csr = rr.remove_csr(csr, keep)[0]
        assert ca.n_reads == csr.n_reads and ca.n_intervals == csr.n_intervals, what
    cb.load_csr(csr, thr)
    g, w = graph(ca, csr.n_reads, engine, cap), graph(cb, csr.n_reads, engine, cap)
    same_graph(g, w, what)
    same_search(ca, cb, csr, what)
    return g, csr


def locus_csr(n_reads, seed, single=False):
    """One locus, a pool of 8 starts: long runs of equal starts (append's one_locus; single: one interval per
    read, so the read count is the interval count)."""
    rng = np.random.default_rng(seed)
    starts = np.arange(8) * 10
    reads = [[(1, int(rng.choice(starts)), 0, 100)] for _ in range(n_reads)] if single else one_locus(n_reads, starts, rng)
    reads = [[(c, s, s + 100, a) for c, s, _, a in r] for r in reads]
    return lists_case(reads, seeds=(seed, seed + 1))[0]


def saved_batch_reads(ctx, hits):
    again = np.empty(max(hits.size, 1), np.int32)
    rc = ctx._L.fslr_search_hits(ctx._h, again.ctypes.data_as(ctypes.c_void_p), hits.size)
    return rc, again[:hits.size]


# ------------------------------------------------------------------ 2. the ends (the smallest cases)
@pytest.mark.parametrize('which', ['first', 'last', 'one_kept'])
def test_ends(ctxs, which):
    csr = synth.generate(300, 8, 5).interval_data().csr()
    keep = np.ones(csr.n_reads, bool)
    if which == 'first':
        keep[0] = False
    elif which == 'last':
        keep[-1] = False
    else:
        keep[:] = False
        keep[137] = True
    _, out = remove_vs_fresh(ctxs, csr, [keep], what=which)
    assert out.n_reads == (1 if which == 'one_kept' else csr.n_reads - 1)


def test_everything_kept_changes_nothing(ctxs):
    ca, _ = ctxs
    csr = synth.generate(500, 8, 3).interval_data().csr()
    ca.load_csr(csr, thr_of(csr))
    want = graph(ca, csr.n_reads)
    _, hits = ca.search(csr.iv_chrom[:50], csr.iv_start[:50], csr.iv_end[:50])
    got = ca.remove_reads(np.ones(csr.n_reads, bool))
    np.testing.assert_array_equal(got, np.arange(csr.n_reads, dtype=np.int32))
    assert ca.n_reads == csr.n_reads and ca.n_intervals == csr.n_intervals
    rc, again = saved_batch_reads(ca, hits)                   # the saved batch still reads: no generation moved
    assert rc == 0
    np.testing.assert_array_equal(again, hits)
    st = ca.run_query(1 - QD, 1 - ND, PT)                     # and the index is still built
    assert st['n_edges'] == want['counts']['n_edges']


# ------------------------------------------------------------------ 1. a random third
@pytest.mark.parametrize('engine', ['walk', 'sweep'])
def test_random_third_removed(ctxs, engine):
    csr = synth.generate(2000, 8, 3).interval_data().csr()
    keep = np.random.default_rng(1).random(csr.n_reads) >= 1 / 3
    g, out = remove_vs_fresh(ctxs, csr, [keep], engine=engine)
    assert g['counts']['engine'] == engine and g['counts']['n_edges'] > 200 and 1200 < out.n_reads < 1450


# ------------------------------------------------------------------ 3. tile seams
def test_every_other_read_across_three_tiles(ctxs):
    csr = locus_csr(2 * T, 30)
    assert 2.5 * T < csr.n_intervals < 3.5 * T
    keep = np.arange(csr.n_reads) % 2 == 0
    remove_vs_fresh(ctxs, csr, [keep])


def test_a_whole_tile_without_a_survivor(ctxs):
    """Data positions [T - 3, 2 T + 3) go: the middle tile writes nothing, its neighbours are partial."""
    csr = locus_csr(3 * T + 40, 31, single=True)
    keep = ~((csr.data_pos >= T - 3) & (csr.data_pos < 2 * T + 3))
    _, out = remove_vs_fresh(ctxs, csr, [keep])
    assert out.n_intervals == csr.n_intervals - (T + 6)


def test_one_tile_kept_of_three(ctxs):
    csr = locus_csr(3 * T + 40, 32, single=True)
    keep = np.zeros(csr.n_reads, bool)
    keep[np.random.default_rng(2).choice(csr.n_reads, T, replace=False)] = True
    _, out = remove_vs_fresh(ctxs, csr, [keep])
    assert out.n_intervals == T


@pytest.mark.parametrize('ni', [T - 1, T, T + 1, 2 * T])
def test_interval_counts_at_the_tile_size(ctxs, ni):
    csr = locus_csr(ni, 33 + ni, single=True)
    assert csr.n_intervals == ni
    keep = np.arange(ni) % 3 != 1
    keep[-1] = False
    remove_vs_fresh(ctxs, csr, [keep], what=f'ni {ni}')
    keep = np.ones(ni, bool)
    keep[ni // 2] = False                                      # one removed element: one tile compacts, the others copy
    remove_vs_fresh(ctxs, csr, [keep], what=f'ni {ni}, one removed')


# ------------------------------------------------------------------ 4. an emptied chromosome
def test_a_middle_chromosome_left_empty(ctxs):
    rng = np.random.default_rng(8)
    reads = [[(c, int(s) * 10, int(s) * 10 + 100, 100) for s in np.sort(rng.choice(8, int(rng.integers(1, 3))))]
             for c in (1, 2, 3) for _ in range(80)]
    csr = mr.resident_data(reads, np.full(240, 1000), np.full(240, 3), shuffle_seed=8).csr()
    keep = np.ones(csr.n_reads, bool)
    keep[np.repeat(np.arange(csr.n_reads), np.diff(csr.read_off))[csr.iv_chrom == 1]] = False
    keep[::7] = False
    g, out = remove_vs_fresh(ctxs, csr, [keep])
    assert out.n_chroms == 3 and not (out.iv_chrom == 1).any() and len(g['edges']) > 100
    q = lambda c: ctxs[0].search(np.full(1, c, np.int32), np.zeros(1, np.int32), np.full(1, 10 ** 6, np.int32))[1]
    assert q(1).size == 0 and q(2).size == int((out.iv_chrom == 2).sum()) > 0


# ------------------------------------------------------------------ 5. the engine flips back
@pytest.mark.parametrize('kind', ['general_threshold', 'zero_aln'])
def test_engine_flag_is_recomputed(ctxs, kind):
    rng = np.random.default_rng(15)
    reads = one_locus(300, np.arange(30) * 5, rng)
    odd = [7, 150, 299]                                         # the only reads with the odd thresholds
    if kind == 'zero_aln':
        for r in odd:
            reads[r] = [(c, s, e, 0) for c, s, e, _ in reads[r]]
    data = mr.resident_data(reads, np.full(300, 1000), np.full(300, 3), shuffle_seed=15)
    csr = data.csr()
    names = np.asarray(data.qnames)[csr.read_qcode]
    odd_rank = np.flatnonzero(np.isin(names, [f'r{r}' for r in odd]))
    assert odd_rank.size == 3
    thr = thr_of(csr)
    keep = np.ones(csr.n_reads, bool)
    keep[odd_rank] = False
    if kind == 'general_threshold':
        thr = np.where(kept_iv(csr, keep), thr, thr_of(csr, 0.0))
        assert (thr < 1).sum() == (~kept_iv(csr, keep)).sum() > 0
    else:
        assert ((thr == FSLR_THR_ZERO_ALN) == ~kept_iv(csr, keep)).all()
    ca, cb = ctxs
    ca.load_csr(csr, thr)
    before = graph(ca, csr.n_reads)
    assert before['counts']['engine'] == 'walk' or before['raised']
    ca.remove_reads(keep)
    out = rr.remove_csr(csr, keep)[0]
    cb.load_csr(out, thr[kept_iv(csr, keep)])
    g, w = graph(ca, out.n_reads), graph(cb, out.n_reads)
    assert w['counts']['engine'] == 'sweep' and not w['raised']
    same_graph(g, w)
    same_search(ca, cb, out)
    ca.set_thresholds(thr_of(out, 0.5))                         # the host's aln_size == 0 marks were compacted too
    cb.set_thresholds(thr_of(out, 0.5))
    same_graph(graph(ca, out.n_reads), graph(cb, out.n_reads))


def test_zero_aln_marks_follow_the_survivors(ctxs):
    """aln_size == 0 intervals stay on kept reads: fslr_set_thresholds checks the marks interval by interval."""
    rng = np.random.default_rng(16)
    reads = one_locus(300, np.arange(30) * 5, rng)
    for r in (3, 120, 280):
        c, s, e, _ = reads[r][-1]
        reads[r][-1] = (c, s, e, 0)
    csr = mr.resident_data(reads, np.full(300, 1000), np.full(300, 3), shuffle_seed=16).csr()
    marked = np.unique(np.repeat(np.arange(csr.n_reads), np.diff(csr.read_off))[csr.iv_aln == 0])
    keep = np.arange(300) % 4 != 2
    keep[marked[0]], keep[marked[1:]] = False, True             # two of the three marked reads stay
    ca, cb = ctxs
    g, out = remove_vs_fresh(ctxs, csr, [keep])
    assert (out.iv_aln == 0).sum() == 2 and (g['counts']['engine'] == 'walk' or g['raised'])
    ca.set_thresholds(thr_of(out, 0.5))
    cb.set_thresholds(thr_of(out, 0.5))
    same_graph(graph(ca, out.n_reads), graph(cb, out.n_reads))


# ------------------------------------------------------------------ 6. the cap binding
def test_cap_binds_on_a_dense_locus(ctxs):
    rng = np.random.default_rng(3)
    reads = [[(2, 500 + int(rng.integers(0, 5)), 700, 200)] for _ in range(200)]
    csr = lists_case(reads)[0]
    keep = np.arange(200) % 10 != 4
    g, _ = remove_vs_fresh(ctxs, csr, [keep], cap=10)
    assert g['cap']['applied'] == 1 and g['counts']['max_fwd'] > 10 and g['cap']['dropped'] > 0


# ------------------------------------------------------------------ 7. round trips
def test_append_then_remove_gives_the_resident_set_back(ctxs):
    ca, cb = ctxs
    data, new_codes = synth_split(1500, 200, seed=21)
    res_d, new_d = split(data, new_codes)
    res = res_d.csr()
    bt = rebased(res_d, res, new_d)
    u = ar.concat_csr(res, bt, n_chroms=bt.n_chroms)
    keep = np.arange(u.n_reads) < res.n_reads
    back = rr.remove_csr(u, keep)[0]
    for f in ('read_off', 'iv_chrom', 'iv_start', 'iv_end', 'data_pos'):       # append_ref and remove_ref agree
        np.testing.assert_array_equal(getattr(back, f), getattr(res, f), err_msg=f)
    ca.load_csr(res, thr_of(res))
    ca.build_index()
    ca.append_csr(bt, thr_of(bt))
    ca.remove_reads(keep)
    cb.load_csr(res, thr_of(res))
    same_graph(graph(ca, res.n_reads), graph(cb, res.n_reads))
    same_search(ca, cb, res)


def test_remove_then_append(ctxs):
    ca, cb = ctxs
    data, new_codes = synth_split(1500, 200, seed=22)
    res_d, new_d = split(data, new_codes)
    res = res_d.csr()
    bt = rebased(res_d, res, new_d)
    keep = np.random.default_rng(4).random(res.n_reads) >= 0.2
    ca.load_csr(res, thr_of(res))
    ca.remove_reads(keep)
    ca.append_csr(bt, thr_of(bt))
    u = ar.concat_csr(rr.remove_csr(res, keep)[0], bt, n_chroms=bt.n_chroms)
    assert ca.n_reads == u.n_reads and ca.n_intervals == u.n_intervals
    cb.load_csr(u, np.concatenate([thr_of(res)[kept_iv(res, keep)], thr_of(bt)]))
    same_graph(graph(ca, u.n_reads), graph(cb, u.n_reads))
    same_search(ca, cb, u)


def test_three_removals_in_a_row(ctxs):
    csr = synth.generate(2000, 8, 7).interval_data().csr()
    rng = np.random.default_rng(5)
    keeps, n = [], csr.n_reads
    for _ in range(3):
        keeps.append(rng.random(n) >= 0.15)
        n = int(keeps[-1].sum())
    _, out = remove_vs_fresh(ctxs, csr, keeps, built=False)
    assert out.n_reads == n


# ------------------------------------------------------------------ 8. refusals and atomicity
def raw_remove(ctx, n, keep, want_map=False):
    k = None if keep is None else np.ascontiguousarray(keep, np.uint8)
    out = np.full(max(int(n), 1), -7, np.int32) if want_map else None
    rc = ctx._L.fslr_remove_reads(ctx._h, int(n), None if k is None else k.ctypes.data_as(ctypes.c_void_p),
                                  None if out is None else out.ctypes.data_as(ctypes.c_void_p))
    return rc, (ctx._L.fslr_last_error(ctx._h) or b'').decode()


def test_invalid_calls_leave_the_context_untouched(ctxs):
    ca, _ = ctxs
    rng = np.random.default_rng(9)
    res = lists_case(one_locus(400, np.arange(50) * 6, rng))[0]
    ca.load_csr(res, thr_of(res))
    want = graph(ca, res.n_reads)
    _, hits = ca.search(res.iv_chrom[:40], res.iv_start[:40], res.iv_end[:40])
    some = np.arange(res.n_reads) % 2 == 0
    bad = [((res.n_reads - 1, some[:-1]), 'the context holds'), ((res.n_reads + 1, np.append(some, True)), 'the context holds'),
           ((res.n_reads, np.zeros(res.n_reads, bool)), 'would leave no reads'), ((res.n_reads, None), 'keep is NULL')]
    for (n, keep), msg in bad:
        rc, text = raw_remove(ca, n, keep, want_map=True)
        assert rc == FSLR_ERR_INVALID and msg in text, (msg, rc, text)
        assert ca.n_reads == res.n_reads
        rc, again = saved_batch_reads(ca, hits)                     # the earlier search batch still reads
        assert rc == 0, msg
        np.testing.assert_array_equal(again, hits)
        st = ca.run_query(1 - QD, 1 - ND, PT)                       # no rebuild: the index is still built
        a, b, I, U = ca.edges(st['n_edges'])
        assert sorted(zip(a.tolist(), b.tolist(), I.tolist(), U.tolist())) == want['edges'], msg
    ca.remove_reads(some)                                           # and a good mask still goes through
    assert ca.n_reads == int(some.sum())
    # what was built and saved belongs to the old reads
    with pytest.raises(_lib.FslrError, match='error 5'):
        ca.run_query(1 - QD, 1 - ND, PT)
    assert saved_batch_reads(ca, hits)[0] == FSLR_ERR_STATE


def test_state_refusals(ctxs):
    ca, _ = ctxs
    rng = np.random.default_rng(29)
    res = lists_case(one_locus(100, np.arange(20) * 3, rng))[0]
    some = np.arange(res.n_reads) % 3 != 0

    def refused(word, n=res.n_reads, built=False):
        hits = None
        if built:
            ca.build_index()
            _, hits = ca.search(res.iv_chrom[:10], res.iv_start[:10], res.iv_end[:10])
        rc, text = raw_remove(ca, n, np.resize(some, n))
        assert rc == FSLR_ERR_STATE and word in text, (word, rc, text)
        if built:                                                    # as it was: the index, the saved batch
            rc, again = saved_batch_reads(ca, hits)
            assert rc == 0, word
            np.testing.assert_array_equal(again, hits)
            np.testing.assert_array_equal(ca.search(res.iv_chrom[:10], res.iv_start[:10], res.iv_end[:10])[1], hits)
    refused('no reads set')
    ca.set_reads(res.read_off, res.read_qlen2, res.read_nal, res.iv_chrom, res.iv_start, res.iv_end, thr_of(res), res.n_chroms)
    refused('without iv_data_pos', built=True)
    long_reads = [[(1, 10 * k, 10 * k + 50, 50) for k in range(70)]] + one_locus(5, np.arange(20) * 3, rng)
    lc = mr.resident_data(long_reads, np.full(6, 1000), np.full(6, 3)).csr()
    ca.load_csr_any(lc, thr_of(lc))
    refused('virtual reads', n=ca.n_reads)
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
    refused('rows', n=3)
    ca.load_csr(res, thr_of(res))                                    # and a plain context removes again
    rc, text = raw_remove(ca, res.n_reads, some)
    assert rc == 0, text


# ------------------------------------------------------------------ 9. DeviceIntervalIndex.remove
def by_name(match_df):
    return sorted((min(a, b), max(a, b), j) for a, b, j in match_df.itertuples(index=False))


def clusters_of(G):
    return sorted(sorted(c) for c in cluster.get_subgraphs(G) if len(c) > 1)


def test_index_remove_against_a_fresh_index():
    data = synth.generate(2000, 8, 41).interval_data()
    args = (PCT, list(CUTOFFS), 10, QD, ND)
    tree = cluster.build_interval_trees(data)
    names = data.qnames[np.asarray(tree.csr.read_qcode)]
    gone = names[np.random.default_rng(6).choice(names.size, 400, replace=False)]
    with pytest.raises(ValueError, match='not a read of this index'):
        tree.remove(qnames=[gone[0], 'no such read'])
    assert tree.csr.n_reads == names.size
    new_rank = tree.remove(qnames=gone)
    np.testing.assert_array_equal(new_rank, rr.rank_map(~np.isin(names, gone)))
    assert tree.source is tree.data and tree.csr.n_reads == names.size - 400
    assert not np.isin(tree.data.qnames[np.asarray(tree.data.qcode)], gone).any()
    m1, G1 = cluster.query_interval_trees(tree, tree.data, *args)
    fresh = cluster.build_interval_trees(data.select(~np.isin(data.qnames[np.asarray(data.qcode)], gone)))
    m2, G2 = cluster.query_interval_trees(fresh, fresh.data, *args)
    assert len(m1) > 300 and by_name(m1) == by_name(m2)
    assert clusters_of(G1) == clusters_of(G2)
    k = np.arange(0, len(tree.data), 7)
    q = (tree.data.chrom[k], tree.data.start[k], tree.data.end[k])
    for x, y in zip(tree.search_batch(*q), fresh.search_batch(*q)):
        np.testing.assert_array_equal(x, y)
    # score_pairs names reads by their new ranks
    left = tree.data.qnames[np.asarray(tree.csr.read_qcode)]
    pa, pb = left[:200], left[1:201]
    s, w = tree.score_pairs(pa, pb, PCT, list(CUTOFFS), QD, ND), fresh.score_pairs(pa, pb, PCT, list(CUTOFFS), QD, ND)
    for f in ('a', 'b', 'I', 'U', 'flags'):
        np.testing.assert_array_equal(getattr(s, f), getattr(w, f), err_msg=f)
    np.testing.assert_array_equal(s.a, np.arange(200))
    with pytest.raises(KeyError):
        tree.score_pairs([gone[0]], [left[0]], PCT, list(CUTOFFS), QD, ND)
    # a removed read may come back
    back = data.select(np.isin(data.qnames[np.asarray(data.qcode)], gone[:50]))
    tree.append(back)
    assert tree.csr.n_reads == names.size - 350
    with pytest.raises(ValueError, match='would leave no reads'):
        tree.remove(keep=np.zeros(tree.csr.n_reads, bool))


def test_python_refusals():
    long_d = mr.resident_data([[(1, 10 * k, 10 * k + 50, 50) for k in range(70)], [(1, 5, 60, 50)]], [1000, 1000], [3, 3])
    long_tree = cluster.build_interval_trees(long_d)
    with pytest.raises(NotImplementedError, match='more than 64 intervals'):
        long_tree.remove(keep=np.array([True, False]))
    with pytest.raises(NotImplementedError, match='does not remove'):
        cluster.MultiGpuIndex.remove(None, keep=[True])
    with pytest.raises(NotImplementedError, match='does not remove'):
        cluster.RowsIndex.remove(None, keep=[True])


def test_golden_fixture_with_reads_removed():
    """mixed_2k_l8 with every fifth read removed on the device: the clusters (as sets of qnames) equal the CPU
    oracle's components on the reduced CSR."""
    data, _, kw = host_prepare('mixed_2k_l8')
    cut = [float(x) for x in kw['jaccard_cutoffs'].split(',')]
    whole = data.csr()
    keep = np.arange(whole.n_reads) % 5 != 2
    reduced = rr.remove_csr(whole, keep)[0]
    o = O.run_core(oracle_from_csr(reduced), kw['overlap'], cut, kw['qlen_diff'], kw['n_alignment_diff'], 10, use_cap=False)
    assert o['stats']['max_fwd'] <= 9                            # the edge cap does not bind
    names = data.qnames[np.asarray(reduced.read_qcode)]
    parent = list(range(reduced.n_reads))                       # the components of the oracle's edges

    def root(x):
        while parent[x] != x:
            parent[x] = x = parent[parent[x]]
        return x
    for a, b in zip(o['edge_a'].tolist(), o['edge_b'].tolist()):
        parent[root(a)] = root(b)
    groups = {}
    for rank, name in enumerate(names.tolist()):
        groups.setdefault(root(rank), []).append(name)
    want = sorted(sorted(g) for g in groups.values() if len(g) > 1)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', cluster.EdgeCapWarning)
        tree = cluster.build_interval_trees(data)
        tree.remove(keep=keep)
        _, G = cluster.query_interval_trees(tree, tree.data, kw['overlap'], cut, 10, kw['qlen_diff'], kw['n_alignment_diff'])
    assert len(want) > 50 and clusters_of(G) == want


# ------------------------------------------------------------------ 10. determinism
def test_two_removals_give_the_same_bytes(ctxs):
    csr = synth.generate(2000, 8, 31).interval_data().csr()
    keep = np.random.default_rng(7).random(csr.n_reads) >= 0.4
    out = []
    for c in ctxs:
        c.load_csr(csr, thr_of(csr))
        c.remove_reads(keep)
        g = graph(c, int(keep.sum()))
        out.append((repr(g['edges']), g['labels'].tobytes(), g['fwd'].tobytes()))
    assert out[0] == out[1]
    same_search(*ctxs, rr.remove_csr(csr, keep)[0])
