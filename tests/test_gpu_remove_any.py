"""fslr_remove_reads_any / DeviceIntervalIndex.remove with reads of more than 64 intervals.

The yardstick of every case is a FRESH context given fslr_set_reads_any (fslr_set_reads once no long read is left)
of the survivors' real CSR (prep.remove_reads_csr).  Both contexts answer the same questions as in
test_gpu_append_any (query, search order, score_pairs_any); everything is compared exactly."""
import ctypes
import warnings

import numpy as np
import pytest

import append_ref as ar
from host_pipeline import host_prepare
from fslr_amd import _lib, cluster
from fslr_amd._lib import FSLR_ERR_INVALID, FSLR_ERR_STATE
from fslr_amd.prep import has_long_reads, remove_reads_csr, split_long_reads, umax_table
from oracle import oracle as O
from test_gpu_parity import oracle_from_csr
from test_gpu_append import CUTOFFS, PCT, thr_of
from test_gpu_append_any import (Intact, saved, case, clusters_of, ctxs, data_of, dense_split, load, locus, long_read,  # noqa: F401
                                 results, rows_context, same, saved_search)

pytestmark = pytest.mark.gpu


def remove_vs_fresh(ctxs, csr, keep, what='', edge_threshold=10, pct=PCT, built=True):
    ca, cb = ctxs
    keep = np.asarray(keep, bool)
    load(ca, csr, pct)
    if built:
        ca.build_index()
    new_rank = ca.remove_reads_any(keep)
    left, want_rank = remove_reads_csr(csr, keep)
    np.testing.assert_array_equal(new_rank, want_rank)
    vn = split_long_reads(left)[0].n_reads if has_long_reads(left) else left.n_reads
    assert ca.n_reads == vn and ca.n_intervals == left.n_intervals
    load(cb, left, pct)
    return same(ca, cb, left, what, edge_threshold, pct), left


def mixed_set(rng, longs=(65, 128, 129, 300)):
    """Short reads with the given long reads spread among them; returns (read lists, ranks of the long reads)."""
    reads = locus(300, rng)
    at = []
    for k, L in enumerate(longs):
        pos = 40 + 60 * k
        reads.insert(pos, long_read(L, (50, 450, 450, 1250)[k % 4], step=4))      # the second and third are near twins
        at.append(pos)
    return reads, at


def csr_and_long_ranks(reads, seed=1):
    """The CSR of the lists and the ranks its long reads got (ranks follow first appearance in the data list)."""
    csr = data_of(reads, seed).csr()
    return csr, np.flatnonzero(np.diff(csr.read_off) > 64)


def test_removing_the_only_long_read_leaves_a_plain_context(ctxs):
    rng = np.random.default_rng(1)
    csr, lg = csr_and_long_ranks(locus(300, rng) + [long_read(70, 100)] + locus(50, rng))
    assert lg.size == 1
    keep = np.ones(csr.n_reads, bool)
    keep[lg] = False
    g, left = remove_vs_fresh(ctxs, csr, keep)
    assert not has_long_reads(left) and g['engine'] in ('sweep', 'walk')   # a plain query again, as on the fresh upload
    # ... and the context takes the short calls again
    ca = ctxs[0]
    more = np.ones(left.n_reads, bool)
    more[::7] = False
    np.testing.assert_array_equal(ca.remove_reads(more), remove_reads_csr(left, more)[1])


def test_removing_a_long_read_between_two_others(ctxs):
    reads, _ = mixed_set(np.random.default_rng(2))
    csr, lg = csr_and_long_ranks(reads)
    keep = np.ones(csr.n_reads, bool)
    keep[lg[1]] = False
    keep[lg[2]] = False
    g, left = remove_vs_fresh(ctxs, csr, keep)
    assert (np.diff(left.read_off) > 64).sum() == lg.size - 2


def test_removing_only_short_reads(ctxs):
    reads, _ = mixed_set(np.random.default_rng(3))
    csr, lg = csr_and_long_ranks(reads)
    keep = np.random.default_rng(3).random(csr.n_reads) < 0.5
    keep[lg] = True
    g, left = remove_vs_fresh(ctxs, csr, keep)
    assert g['long_pair_edges'] > 0


def test_keeping_one_long_read_only(ctxs):
    reads, _ = mixed_set(np.random.default_rng(4))
    csr, lg = csr_and_long_ranks(reads)
    keep = np.zeros(csr.n_reads, bool)
    keep[lg[2]] = True
    g, left = remove_vs_fresh(ctxs, csr, keep)
    assert left.n_reads == 1 and g['edges'] == []


def test_a_mask_that_empties_a_read_tile_and_a_data_tile(ctxs):
    """Reads 256 .. 511 go (a whole 256-read tile of the maps) together with every read that has an interval among
    data positions 1024 .. 2047 (a whole 1024-position tile of the data-order compaction)."""
    rng = np.random.default_rng(5)
    reads = locus(900, rng, 0, 20000) + [long_read(200, 10, step=90), long_read(70, 15000, step=20)]
    csr, lg = csr_and_long_ranks(reads)
    keep = np.ones(csr.n_reads, bool)
    keep[256:512] = False
    r_of = np.repeat(np.arange(csr.n_reads), np.diff(csr.read_off))
    keep[r_of[(csr.data_pos >= 1024) & (csr.data_pos < 2048)]] = False
    assert keep.sum() > 100
    remove_vs_fresh(ctxs, csr, keep, built=False)


def test_everything_kept_moves_no_generation(ctxs):
    ca, cb = ctxs
    reads, _ = mixed_set(np.random.default_rng(6))
    csr, _ = csr_and_long_ranks(reads)
    load(ca, csr)
    ca.build_index()
    q = (csr.iv_chrom[:50], csr.iv_start[:50], csr.iv_end[:50])
    _, hits = ca.search(*q)
    np.testing.assert_array_equal(ca.remove_reads_any(np.ones(csr.n_reads, bool)), np.arange(csr.n_reads))
    rc, again = saved_search(ca, hits)                               # the saved batch is still readable
    assert rc == 0
    np.testing.assert_array_equal(again, hits)
    load(cb, csr)
    same(ca, cb, csr)


def test_append_then_remove_and_remove_then_append(ctxs):
    ca, cb = ctxs
    rng = np.random.default_rng(7)
    res, bt = case(locus(200, rng) + [long_read(129, 30), long_read(66, 900)], locus(60, rng) + [long_read(100, 300), long_read(64, 5)])
    load(ca, res)
    first = results(ca, res)
    ca.append_csr_any(bt, thr_of(bt))
    u = ar.concat_csr(res, bt, n_chroms=bt.n_chroms)
    keep = np.arange(u.n_reads) < res.n_reads
    ca.remove_reads_any(keep)
    assert ca.n_reads == split_long_reads(res)[0].n_reads and ca.n_intervals == res.n_intervals
    assert results(ca, res) == first
    # remove some resident reads (a long one among them), then append the batch
    lg = np.flatnonzero(np.diff(res.read_off) > 64)
    keep = np.arange(res.n_reads) % 4 != 1
    keep[lg[0]] = False
    keep[lg[1]] = True
    ca.remove_reads_any(keep)
    left, _ = remove_reads_csr(res, keep)
    ca.append_csr_any(bt, thr_of(bt))
    v = ar.concat_csr(left, bt, n_chroms=bt.n_chroms)
    load(cb, v)
    same(ca, cb, v)


def test_a_surviving_long_read_with_an_aln_size_zero_interval(ctxs):
    rng = np.random.default_rng(8)
    zero = long_read(80, 200, step=5)
    zero[70] = (1, zero[70][1], zero[70][2], 0)                        # aln_size 0 in a further chunk
    csr, lg = csr_and_long_ranks(locus(200, rng) + [zero, long_read(90, 600)] + locus(40, rng))
    assert (csr.iv_aln == 0).sum() == 1
    zr = np.repeat(np.arange(csr.n_reads), np.diff(csr.read_off))[csr.iv_aln == 0][0]
    keep = np.arange(csr.n_reads) % 3 != 0
    keep[lg] = False
    keep[zr] = True
    g, left = remove_vs_fresh(ctxs, csr, keep)
    assert (left.iv_aln == 0).sum() == 1 and (np.diff(left.read_off) > 64).sum() == 1
    # the survivors' mark moved with its interval (the host checks it against the thresholds the query installs), and
    # the pairs that meet the interval raise as the reference's calculate_overlap does, on both contexts alike
    assert g.get('raised') and g['zd_pairs'] > 0


def test_a_binding_cap(ctxs):
    a, b = dense_split(np.random.default_rng(9))
    csr, lg = csr_and_long_ranks(a + b)
    keep = np.arange(csr.n_reads) % 5 != 2
    keep[lg[0]] = True
    g, left = remove_vs_fresh(ctxs, csr, keep, edge_threshold=3)
    assert g['cap']['applied'] == 1


def raw_remove_any(ctx, n, keep):
    k = np.ascontiguousarray(keep, dtype=np.uint8)
    out = np.empty(max(int(n), 1), np.int32)
    rc = ctx._L.fslr_remove_reads_any(ctx._h, int(n), k.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    return rc, (ctx._L.fslr_last_error(ctx._h) or b'').decode()


def test_refusals_leave_the_index_and_the_saved_batches(ctxs):
    ca, _ = ctxs
    reads, _ = mixed_set(np.random.default_rng(10))
    csr, lg = csr_and_long_ranks(reads)
    some = np.arange(csr.n_reads) % 3 != 0
    load(ca, csr)
    want = results(ca, csr)
    state = Intact(ca, csr)
    rc, text = raw_remove_any(ca, csr.n_reads, np.zeros(csr.n_reads, bool))
    assert rc == FSLR_ERR_INVALID and 'would leave no reads' in text
    state.check()
    rc, text = raw_remove_any(ca, ca.n_reads, np.resize(some, ca.n_reads))          # the virtual count is not the real one
    assert rc == FSLR_ERR_INVALID and 'but the context holds' in text
    state.check()
    ca.set_chrom_filter(np.ones(csr.n_chroms, bool))
    before = saved(ca, state)                                    # (fslr_search itself refuses under a filter)
    rc, text = raw_remove_any(ca, csr.n_reads, some)
    assert rc == FSLR_ERR_STATE and 'filter' in text
    assert saved(ca, state) == before                            # the saved batches as the filter left them
    ca.set_chrom_filter(None)
    assert results(ca, csr) == want
    v, vreal, vbase, rlen = split_long_reads(csr)
    ca.load_csr(v, thr_of(v))
    ca.set_long_reads(csr.n_reads, vreal, vbase, rlen, umax_table(list(CUTOFFS), int(rlen.max())))
    own = Intact(ca, csr)
    rc, text = raw_remove_any(ca, csr.n_reads, some)
    assert rc == FSLR_ERR_STATE and 'fslr_set_long_reads' in text, text
    own.check()
    q, hits = rows_context(ca)
    rc, text = raw_remove_any(ca, 3, [1, 0, 1])
    assert rc == FSLR_ERR_STATE and 'rows' in text
    rc, again = saved_search(ca, hits)
    assert rc == 0
    np.testing.assert_array_equal(again, hits)
    np.testing.assert_array_equal(ca.search(*q)[1], hits)
    load(ca, csr)
    rc, text = raw_remove_any(ca, csr.n_reads, some)
    assert rc == 0, text


def test_two_runs_give_the_same_bytes(ctxs):
    reads, _ = mixed_set(np.random.default_rng(11))
    csr, lg = csr_and_long_ranks(reads)
    keep = np.random.default_rng(11).random(csr.n_reads) < 0.6
    keep[lg[:2]] = [True, False]
    left, _ = remove_reads_csr(csr, keep)
    out = []
    for c in ctxs:
        load(c, csr)
        c.remove_reads_any(keep)
        g = results(c, left)
        _, hits = c.search(left.iv_chrom[::3], left.iv_start[::3], left.iv_end[::3])
        out.append((repr(g), hits.tobytes()))
    assert out[0] == out[1]


def test_index_remove_on_the_long_read_fixture_against_a_fresh_index_and_the_oracle():
    data, _, kw = host_prepare('longreads_400')
    cut = [float(x) for x in kw['jaccard_cutoffs'].split(',')]
    args = (kw['overlap'], cut, 10, kw['qlen_diff'], kw['n_alignment_diff'])
    whole = data.csr()
    keep = np.arange(whole.n_reads) % 4 != 1
    lg = np.flatnonzero(np.diff(whole.read_off) > 64)
    assert lg.size > 2
    keep[lg[0]], keep[lg[1]] = False, True
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', cluster.EdgeCapWarning)
        tree = cluster.build_interval_trees(data)
        new_rank = tree.remove_any(keep=keep)
        np.testing.assert_array_equal(new_rank, remove_reads_csr(whole, keep)[1])
        fresh = cluster.build_interval_trees(tree.data)
        _, G1 = cluster.query_interval_trees(tree, tree.data, *args)
        _, G2 = cluster.query_interval_trees(fresh, fresh.data, *args)
    assert clusters_of(G1) == clusters_of(G2)
    k = np.arange(0, len(tree.data), 5)
    q = (tree.data.chrom[k], tree.data.start[k], tree.data.end[k])
    for x, y in zip(tree.search_batch(*q), fresh.search_batch(*q)):
        np.testing.assert_array_equal(x, y)
    o = O.run_core(oracle_from_csr(tree.csr), kw['overlap'], cut, kw['qlen_diff'], kw['n_alignment_diff'], 10)
    names = tree.data.qnames[np.asarray(tree.csr.read_qcode)]
    groups = {}
    for rank, comp in enumerate(o['comp'][:tree.csr.n_reads].tolist()):
        if comp >= 0:
            groups.setdefault(comp, []).append(names[rank])
    assert len(groups) > 0 and clusters_of(G1) == sorted(sorted(g) for g in groups.values())
    # match_reads_any with the removed reads as query reads, then the round trip: they come back as a batch
    gone = data.select(~np.isin(np.asarray(data.qcode), np.asarray(whole.read_qcode)[keep]))
    margs = (kw['overlap'], cut, kw['qlen_diff'], kw['n_alignment_diff'])
    rows = lambda r: sorted(map(tuple, r.to_frame().itertuples(index=False)))
    r1, r2 = tree.match_reads_any(gone, *margs), fresh.match_reads_any(gone, *margs)
    assert len(r1.partner) > 0 and rows(r1) == rows(r2)
    for f in ('offsets', 'partner', 'I', 'U', 'flags'):              # the same rank order here: the same rows
        np.testing.assert_array_equal(getattr(r1, f), getattr(r2, f), err_msg=f)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', cluster.EdgeCapWarning)
        tree.append_any(gone)
        assert tree.csr.n_reads == whole.n_reads and len(tree.data) == len(data)
        again = cluster.build_interval_trees(tree.data)
        m3, G3 = cluster.query_interval_trees(tree, tree.data, *args)
        m4, G4 = cluster.query_interval_trees(again, again.data, *args)
    assert clusters_of(G3) == clusters_of(G4)
    pairs = lambda m: sorted((min(a, b), max(a, b), j) for a, b, j in m.itertuples(index=False))
    assert len(m3) > 0 and pairs(m3) == pairs(m4)
