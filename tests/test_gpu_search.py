"""The batched interval search on the device index (fslr_search / DeviceIntervalIndex.search_batch):
offsets, data positions and counts equal the brute force of search_ref (predicate and order of the
superintervals stand-in, cluster.py:201), at the kernels' own boundaries: 64-position pieces,
256-position prefix-max tiles, 1024-position range blocks."""
import ctypes

import numpy as np
import pytest

import search_ref as sr
from fslr_amd import _lib, cluster, synth
from fslr_amd.prep import IntervalData, fold_overlap_threshold, pass_table
from host_pipeline import host_prepare

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def check(idx, qc, qs, qe):
    d = idx.data
    want_off, want_pos = sr.brute_force(d.chrom, d.start, d.end, qc, qs, qe)
    off, pos = idx.search_batch(qc, qs, qe)
    assert off.dtype == np.int64 and pos.dtype == np.int64
    np.testing.assert_array_equal(off, want_off)
    np.testing.assert_array_equal(pos, want_pos)
    np.testing.assert_array_equal(idx.count_batch(qc, qs, qe), np.diff(want_off))
    return off, pos


def random_input(rng, n=5000):
    """n intervals with unique starts on chromosomes 3, 11 and 12; 12 holds a single interval."""
    start = rng.choice(2_000_000, n, replace=False)
    end = start + rng.integers(0, 3000, n)
    end[::97] += 150_000                                        # a few long ones: backward spans over tiles
    chrom = np.where(rng.random(n) < 0.6, 3, 11)
    chrom[n // 2] = 12
    return sr.make_data(chrom, start, end)


def test_random(ctx):
    rng = np.random.default_rng(101)
    data = random_input(rng)
    idx = cluster.build_interval_trees(data, ctx=ctx)
    n = len(data)
    pick = rng.integers(0, n, 2400)
    c, s, e = data.chrom[pick], data.start[pick], data.end[pick]
    k = 400
    qc = np.concatenate([c[:k], c[k:2 * k], c[2 * k:3 * k], c[3 * k:4 * k], c[4 * k:5 * k], c[5 * k:]])
    qs = np.concatenate([s[:k] + rng.integers(0, 50, k),        # point queries
                         e[k:2 * k],                            # qs == a stored end
                         s[2 * k:3 * k] - rng.integers(1, 5000, k),
                         s[3 * k:4 * k] + 700,                  # qs > qe
                         s[4 * k:5 * k] - rng.integers(0, 2000, k),
                         rng.integers(0, 2_100_000, 2400 - 5 * k)])
    qe = np.concatenate([qs[:k],
                         e[k:2 * k] + rng.integers(0, 3, k),
                         s[2 * k:3 * k],                        # qe == a stored start
                         s[3 * k:4 * k],
                         e[4 * k:5 * k] + rng.integers(0, 2000, k),
                         rng.integers(0, 2_100_000, 2400 - 5 * k)])
    big = 1 << 40
    special = [  # (chrom, qs, qe): left of, right of and covering a chromosome; absent chromosomes; far coordinates
        (3, -5000, -1), (3, -1, 0), (3, 2_200_000, 2_300_000), (3, 0, 2_200_000), (3, -big, big),
        (11, -7, int(data.start[data.chrom == 11].min())), (11, int(data.end[data.chrom == 11].max()), big),
        (11, (1 << 30) + 5, (1 << 31) + 7), (11, -big, -big + 3), (12, -3, 1 << 31), (12, 0, 0),
        (12, int(data.end[data.chrom == 12][0]), 1 << 30), (5, 0, 2_000_000), (-1, 0, 2_000_000), (1 << 20, 0, 10)]
    fill = 3000 - 2400 - len(special)
    qc = np.concatenate([qc, [x[0] for x in special], rng.choice([3, 11, 12, 4], fill)])
    qs = np.concatenate([qs, [x[1] for x in special], rng.integers(-1000, 2_100_000, fill)])
    qe = np.concatenate([qe, [x[2] for x in special], rng.integers(-1000, 2_200_000, fill)])
    assert qc.size == 3000
    off, _ = check(idx, qc, qs, qe)
    assert off[-1] > 10_000


def test_ties_and_determinism(ctx):
    """Runs of equal (chrom, start) of 2 .. 1100 intervals, cut at every distinct end; twice, for the
    same bytes."""
    data, (qc, qs, qe) = sr.tie_input()
    idx = cluster.build_interval_trees(data, ctx=ctx)
    off, pos = check(idx, qc, qs, qe)
    assert np.diff(off).max() >= 1100
    off2, pos2 = idx.search_batch(qc, qs, qe)
    assert off.tobytes() == off2.tobytes() and pos.tobytes() == pos2.tobytes()


def test_ties_item_list_not_start_sorted():
    """The reference's own list type, not in start order (the (chrom, start) sort path of the index
    build, no data positions on the device): the same contract in data positions."""
    data, (qc, qs, qe) = sr.tie_input(seed=8)
    items = list(data)[::-1]
    idx = cluster.build_interval_trees(items)
    try:
        assert not idx.csr.start_sorted
        check(idx, qc, qs, qe)
        assert [it.index for it in idx[7].search_values(int(qs[0]), int(qe[0]))] == \
            [items[p].index for p in idx[7].search_idxs(int(qs[0]), int(qe[0])).tolist()]
    finally:
        idx.ctx.close()


def test_reach(ctx):
    """One interval per chromosome spans it and sits first: every backward span crosses all tiles."""
    rng = np.random.default_rng(7)
    chrom, start, end = [], [], []
    for c in (1, 2):
        chrom += [c] * 2501
        s = np.sort(rng.choice(np.arange(1, 5_000_000), 2500, replace=False))
        start += [0] + s.tolist()
        end += [5_000_000] + (s + rng.integers(10, 400, 2500)).tolist()
    data = sr.make_data(chrom, start, end)
    idx = cluster.build_interval_trees(data, ctx=ctx)
    nq = 600
    qc = rng.integers(1, 3, nq)
    qs = rng.integers(4_900_000, 5_000_200, nq)
    qe = qs + rng.integers(0, 5000, nq)
    off, _ = check(idx, qc, qs, qe)
    assert (np.diff(off)[qs <= 5_000_000] >= 1).all()


@pytest.mark.parametrize('n', [1, 255, 256, 257])
def test_tiny_and_empty(ctx, n):
    rng = np.random.default_rng(n)
    start = np.sort(rng.choice(100_000, n, replace=False))
    data = sr.make_data(np.ones(n, np.int64), start, start + rng.integers(0, 2000, n))
    idx = cluster.build_interval_trees(data, ctx=ctx)
    off, pos = idx.search_batch(np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64))
    assert off.tolist() == [0] and pos.size == 0 and idx.count_batch([], [], []).size == 0
    qs = rng.integers(-50, 103_000, 300)
    off, _ = check(idx, np.ones(300, np.int64), qs, qs + rng.integers(0, 3000, 300))
    assert off[-1] > 0
    off, pos = check(idx, [1, 1, 2, 1], [200_000, -9, 0, 5], [300_000, -2, 100_000, 4 if start[0] > 4 else -1])
    assert off[-1] == 0 and pos.size == 0                       # every query misses


@pytest.mark.parametrize('first', ['search_values', 'count_batch', 'search_batch'])
def test_first_search_of_a_fresh_context_misses(first):
    """The very first search of a context finds nothing (a look at an empty locus right after
    build_interval_trees): no piece buffer exists yet.  Zero offsets, no hits; then a hitting search."""
    start = np.arange(300, dtype=np.int64) * 100 + 10_000
    data = sr.make_data(np.full(300, 4, np.int64), start, start + 50)
    idx = cluster.build_interval_trees(data)                    # its own, fresh context
    try:
        qc, qs, qe = [4, 4, 4], [0, 10_060, 900_000], [9_999, 10_090, 900_500]     # left of, between, right of
        if first == 'search_values':
            assert idx[4].search_values(10_060, 10_090) == []
            assert idx[4].search_idxs(0, 9_999).size == 0 and idx[4].count(900_000, 900_500) == 0
        elif first == 'count_batch':
            assert idx.count_batch(qc, qs, qe).tolist() == [0, 0, 0]
        off, pos = idx.search_batch(qc, qs, qe)
        assert off.tolist() == [0, 0, 0, 0] and pos.size == 0 and pos.dtype == np.int64
        assert idx.count_batch(qc, qs, qe).tolist() == [0, 0, 0]
        check(idx, [4, 4, 4, 9], [0, 10_050, 10_051, 0], [10_010, 10_100, 10_099, 50_000])
        assert [it.start for it in idx[4].search_values(10_050, 10_100)] == [10_100, 10_000]
    finally:
        idx.ctx.close()


def test_saved_batch_belongs_to_one_index_build():
    """fslr_search_hits after another fslr_build_index: FSLR_ERR_STATE, nothing written, until the next
    fslr_search."""
    start = np.arange(500, dtype=np.int64) * 10
    idx = cluster.build_interval_trees(sr.make_data(np.ones(500, np.int64), start, start + 25))
    c = idx.ctx
    try:
        dense = idx._dense_chroms([1, 1])
        total = c._search(dense, [0, 100], [50, 130], None)
        assert total > 0
        c.build_index()
        buf = np.full(total, -7, np.int32)
        assert c._L.fslr_search_hits(c._h, buf.ctypes.data_as(ctypes.c_void_p), total) == _lib.FSLR_ERR_STATE
        assert (buf == -7).all()
        check(idx, [1, 1], [0, 100], [50, 130])
    finally:
        c.close()


def test_self_join(ctx):
    """Every stored interval as its own query; each count is 1 + n_fwd + the backward hits, the identity
    the index build states (index.hip)."""
    data = synth.generate(3000, 16, 11).interval_data()
    idx = cluster.build_interval_trees(data, ctx=ctx)
    off, _ = check(idx, data.chrom, data.start, data.end)
    want = np.empty(len(data), np.int64)
    for c in np.unique(data.chrom):
        sel = np.flatnonzero(data.chrom == c)                   # (chrom, start) order, ties in data order
        s, e = data.start[sel], data.end[sel]
        n_fwd = np.searchsorted(s, e, side='right') - np.arange(sel.size) - 1
        bwd = np.array([(e[:q] >= s[q]).sum() for q in range(sel.size)])
        want[sel] = 1 + n_fwd + bwd
    np.testing.assert_array_equal(np.diff(off), want)


def reference_loop(tree, data, overlap, cutoffs, edge_threshold, qlen_diff, diff):
    """cluster.py:197-224 restated: the candidates come from tree[chrom].search_values, the predicates
    from the CPU oracle."""
    from oracle import oracle as O
    lists = {}
    for itv in data:
        lists.setdefault(itv.qname, []).append(itv)
    cols = {q: [(x.chrom, x.start, x.end, x.aln_size) for x in l] for q, l in lists.items()}
    seen, match = set(), set()
    for query_key, list1 in lists.items():
        edges = 0
        for itv in list1:
            for o_data in tree[itv.chrom].search_values(itv.start, itv.end):
                if o_data.qname == query_key:
                    continue
                b = tuple(sorted((o_data.qname, query_key)))
                if b in seen:
                    continue
                seen.add(b)
                if O.lengths_differ(itv.qlen2, o_data.qlen2, itv.n_alignments, o_data.n_alignments, qlen_diff, diff):
                    continue
                I, U = O.jaccard_lists(cols[query_key], cols[o_data.qname], overlap)
                if I == 0:
                    continue
                target = cutoffs[I - 1] if I - 1 < len(cutoffs) else cutoffs[-1]
                if I / U >= target:
                    match.add((query_key, o_data.qname, I / U))
                    edges += 1
                if edges >= edge_threshold:
                    break
    return match


def test_reference_loop_runs_unchanged_on_the_index():
    """capbind_1500 (the cap binds): the reference's pair loop over our tree gives query_interval_trees'
    edges: the search order is the one the cap replay uses."""
    data, _, kw = host_prepare('capbind_1500')
    cut = [float(x) for x in kw['jaccard_cutoffs'].split(',')]
    tree = cluster.build_interval_trees(data)
    try:
        m, G = cluster.query_interval_trees(tree, data, kw['overlap'], cut, 10, kw['qlen_diff'],
                                            kw['n_alignment_diff'])
        assert G.stats['cap']['applied'] == 1 and G.stats['cap']['capped'] > 0
        got = reference_loop(tree, data, kw['overlap'], cut, 10, kw['qlen_diff'], kw['n_alignment_diff'])
        assert got == set(map(tuple, m.itertuples(index=False)))
        assert isinstance(next(iter(tree[data.chrom[0]].search_values(0, 1 << 30))), cluster.IntervalItem)
        assert tree['no such chromosome'].search_values(0, 10) == [] and tree[-4].count(0, 10) == 0
        assert sorted(tree.keys()) == sorted(set(data.chrom.tolist())) and len(tree.items()) == len(tree.keys())
    finally:
        tree.ctx.close()


def test_rows_upload_path():
    """An index built from rows on the device (fslr_rows_upload + fslr_set_reads_rows): positions of the
    `data` list, through the CSR the device made."""
    rng = np.random.default_rng(33)
    n_reads = 900
    L = rng.integers(1, 5, n_reads)
    q = np.repeat(np.arange(n_reads, dtype=np.int64), L)
    m = q.size
    start = rng.integers(0, 300, m) * 400 + rng.integers(0, 3, m)          # many equal starts
    size = rng.integers(100, 1500, m)
    rows = dict(chrom=rng.integers(1, 4, m).astype(np.int64), start=start.astype(np.int64),
                end=(start + size).astype(np.int64), aln=size.astype(np.int64), qcode=q,
                nal=np.repeat(L, L).astype(np.int64), qlen2=np.full(m, 5000, np.int64))
    order = np.argsort(rows['start'], kind='stable').astype(np.int64)
    data = IntervalData(chrom=rows['chrom'][order], start=rows['start'][order], end=rows['end'][order],
                        aln_size=rows['aln'][order], qcode=q[order],
                        qnames=np.asarray([f'q{k}' for k in range(n_reads)], dtype=object),
                        n_alignments=rows['nal'][order], qlen2=rows['qlen2'][order],
                        middle=(rows['aln'] // 2 + rows['start'])[order], index=order)
    c = _lib.Context(0)
    try:
        c.rows_upload(rows, n_reads, 4)
        info = c.set_reads_rows(order, None, 0.8)
        idx = cluster.RowsIndex(data, cluster.RowsCSR(c, info), c, 0.8)
        check(idx, data.chrom, data.start, data.end)
        qs = rng.integers(-100, 125_000, 500)
        check(idx, rng.integers(0, 5, 500), qs, qs + rng.integers(0, 3000, 500))
    finally:
        c.close()


def test_long_read_upload_path():
    """One read of 150 intervals (fslr_set_reads_any splits it into 64-interval chunks): positions of
    the real input's `data` list."""
    rng = np.random.default_rng(44)
    n = 700
    qcode = np.concatenate([np.zeros(150, np.int64), 1 + rng.integers(0, 200, n - 150)])
    start = rng.integers(0, 200, n) * 500 + rng.integers(0, 2, n)
    data = sr.make_data(rng.integers(1, 3, n), start, start + rng.integers(50, 2500, n), qcode=qcode, shuffle_seed=2)
    idx = cluster.build_interval_trees(data)
    try:
        assert idx.long is not None and idx.long.max() == 150
        check(idx, data.chrom, data.start, data.end)
    finally:
        idx.ctx.close()


def test_search_leaves_the_query_state_alone():
    s = synth.generate(3000, 16, 11)
    data = s.interval_data()
    idx = cluster.build_interval_trees(data)
    c = idx.ctx
    try:
        c.set_thresholds(fold_overlap_threshold(idx.csr.iv_aln, 0.8))
        c.reserve_edges(12 * idx.csr.n_reads)
        pt = pass_table([1, 1, 0.66, 0.66, 0.66, 0.5])

        def raw():
            return [x.tobytes() for x in c.edges(c.stats()['n_edges'])]

        def state():                                # a query appends its edges in no fixed order: as a set
            a, b, I, U = c.edges(c.stats()['n_edges'])
            return sorted(zip(a.tolist(), b.tolist(), I.tolist(), U.tolist())), c.labels().tobytes(), \
                c.fwd_degree().tobytes()
        c.run(0.96, 0.75, pt)
        before, before_raw = state(), raw()
        assert len(before[0]) > 0
        for k in range(3):
            sel = slice(k, None, 3)
            check(idx, data.chrom[sel], data.start[sel], data.end[sel])
        assert raw() == before_raw and state() == before      # the edges in HBM: the same bytes
        c.run(0.96, 0.75, pt)
        assert state() == before
        # a too-small capacity: FSLR_ERR_INVALID with the needed count, and the next search succeeds
        off, pos = idx.search_batch(data.chrom[:50], data.start[:50], data.end[:50])
        total = int(off[-1])
        buf = np.full(total, -7, np.int32)
        assert c._L.fslr_search_hits(c._h, buf.ctypes.data_as(ctypes.c_void_p), total - 1) == _lib.FSLR_ERR_INVALID
        assert str(total) in c._L.fslr_last_error(c._h).decode() and (buf == -7).all()
        check(idx, data.chrom[:50], data.start[:50], data.end[:50])
        # a chromosome filter: the index is partial and cannot answer
        c.set_chrom_filter(np.arange(idx.csr.n_chroms) % 2 == 0)
        c.build_index()
        with pytest.raises(_lib.FslrError, match=f'fslr error {_lib.FSLR_ERR_STATE}.*filter'):
            idx.search_batch(data.chrom[:5], data.start[:5], data.end[:5])
        c.set_chrom_filter(None)
        with pytest.raises(_lib.FslrError, match=f'fslr error {_lib.FSLR_ERR_STATE}.*fslr_build_index'):
            idx.count_batch(data.chrom[:5], data.start[:5], data.end[:5])
        c.build_index()
        check(idx, data.chrom[:5], data.start[:5], data.end[:5])
    finally:
        c.close()
