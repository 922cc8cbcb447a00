"""Cluster junctions on the device (fslr_cluster_junctions, fslr_get_cluster_junctions) against
tests/junctions_ref.py, which tests/test_junctions_ref.py pins to hand-worked cases.  Clusters come from host label
vectors, so read lengths, lane groups, row counts and segment sizes are exact; the query keys and strand bits are
made per CSR interval.  Every comparison is exact."""
import os

import numpy as np
import pandas as pd
import pytest

import fixtures as fx
import junctions_ref as jr
import loci_ref as lr
import search_ref as sr
from fslr_amd import _lib, cluster
from test_gpu_loci import fixture_membership, query, run_cli

pytestmark = pytest.mark.gpu

INVALID = f'fslr error {_lib.FSLR_ERR_INVALID}'
STATE = f'fslr error {_lib.FSLR_ERR_STATE}'
B = 256                        # the reduce kernels' block: segments of B - 1, B, B + 1 and 2 B + 1 straddle blocks
WINDOW = 10000


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def build(ctx, lens, seed=0, n_chroms=3, share=3, span=9000, width=300):
    """Reads of the given interval counts, rank k = the k-th of ``lens``: ``share`` consecutive reads lie in one
    window, so their intervals merge into common loci here and there (and a read meets its own locus again)."""
    rng = np.random.default_rng(seed)
    chrom, start, end, read = [], [], [], []
    for k, n in enumerate(lens):
        base = (k // share) * WINDOW
        starts = [base + k % share] + (base + share + rng.integers(0, span, n - 1)).tolist()
        for s in starts:
            chrom.append(int(rng.integers(0, n_chroms))), start.append(int(s)), read.append(k)
            end.append(int(s) + int(rng.integers(0, width)))
    idx = cluster.build_interval_trees(sr.make_data(chrom, start, end, qcode=read), ctx=ctx)
    assert np.diff(idx.csr.read_off).tolist() == list(lens)           # the ranks are the order of ``lens``
    return idx


def keys_of(csr, mode, rng):
    n, off = csr.n_intervals, np.asarray(csr.read_off, np.int64)
    j = np.arange(n) - np.repeat(off[:-1], np.diff(off))              # the interval's place in its read
    if mode == 'ascending':
        return j.astype(np.int32)
    if mode == 'descending':
        return (-j).astype(np.int32)
    if mode == 'random':
        return rng.integers(-40, 40, n).astype(np.int32)              # with ties
    if mode == 'equal':
        return np.full(n, 7, np.int32)
    if mode == 'negative':
        return (-(1 << 31) + rng.integers(0, 50, n)).astype(np.int32)
    assert mode == 'extreme'
    return rng.choice(np.asarray([-(1 << 31), -1, 0, (1 << 31) - 1], np.int64), n).astype(np.int32)


def groups_of(n, size, rng=None, alone=()):
    """Labels: consecutive groups of ``size`` reads (shuffled membership with rng), ranks in ``alone`` left out."""
    who = np.asarray([r for r in range(n) if r not in set(alone)], np.int64)
    if rng is not None:
        who = rng.permutation(who)
    lab = np.arange(n, dtype=np.int32)
    for g in range(0, who.size, size):
        m = who[g:g + size]
        if m.size >= 2:
            lab[m] = m.min()
    return lab


def device_rows(c, qkey, rev=None, labels=None, loci=True):
    if labels is not None:
        c.cluster_table(labels)
    if loci:
        c.cluster_loci()
    return dict(zip(('off',) + jr.COLUMNS, c.cluster_junctions(qkey, rev)))


def same_rows(got, want):
    for k in ('off',) + jr.COLUMNS:
        assert got[k].dtype == want[k].dtype, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def check(idx, labels, qkey, rev=None):
    want = jr.junctions_of_csr(idx.csr, labels, qkey, rev)
    same_rows(device_rows(idx.ctx, qkey, rev, labels), want)
    return want


# ------------------------------------------------------------------ 1. lane groups and chains
SEAM_LENS = (2, 15, 16, 17, 32, 33, 63, 64)


@pytest.mark.parametrize('mode', ['ascending', 'descending', 'random', 'equal', 'negative', 'extreme'])
def test_read_lengths_alone_in_a_wavefront(ctx, mode):
    """Each seam length with three one-interval reads behind it: the long read decides its wavefront's group width
    alone.  The one-interval reads are clustered with it (they give loci, no observations)."""
    lens = [x for n in SEAM_LENS for x in (n, 1, 1, 1)] * 2
    idx = build(ctx, lens, seed=len(mode), share=4)
    rng = np.random.default_rng(1)
    want = check(idx, groups_of(len(lens), 8), keys_of(idx.csr, mode, rng), rng.integers(0, 2, idx.csr.n_intervals).astype(np.uint8))
    assert int(want['n_obs'].sum()) == 2 * sum(n - 1 for n in SEAM_LENS)


@pytest.mark.parametrize('rev_mode', ['null', 'ones', 'random'])
def test_read_lengths_mixed_four_to_a_wavefront(ctx, rev_mode):
    """Quads that keep 16-lane groups, quads one read pushes to 32 or 64 lanes, reads alone and one-interval reads
    between them, and a last quad that is not full."""
    rng = np.random.default_rng(11)
    quads = [(2, 15, 16, 3), (16, 16, 16, 16), (17, 2, 2, 2), (5, 32, 1, 16), (33, 16, 2, 1), (2, 3, 63, 4),
             (64, 64, 64, 64), (1, 1, 1, 1), (64, 1, 33, 17), (16, 17, 32, 33), (9, 2)]
    lens = [n for q in quads for n in q] * 3
    idx = build(ctx, lens, seed=3)
    n = idx.csr.n_intervals
    rev = {'null': None, 'ones': np.ones(n, np.uint8), 'random': rng.integers(0, 2, n).astype(np.uint8)}[rev_mode]
    lab = groups_of(len(lens), 5, rng, alone=range(4, len(lens), 9))
    want = check(idx, lab, keys_of(idx.csr, 'random', rng), rev)
    assert len(want['n_obs']) > 500 and (want['locus_a'] == want['locus_b']).any()        # self-junctions too


def test_reads_and_their_reverse_complements(ctx):
    """A cluster that holds every read twice.  With the copies read from the other strand (order reversed, every
    strand bit flipped) the rows are the same bytes as with the copies as they are, and every count is even."""
    rng = np.random.default_rng(4)
    reads = []
    for r in range(40):
        n = int(rng.integers(2, 20))
        reads.append([(int(rng.integers(0, 2)), int(s), int(s) + int(rng.integers(0, 300))) for s in
                      rng.choice(6000, n, replace=False)])
    idx = index_of(ctx, reads + reads)
    csr = idx.csr
    off = np.asarray(csr.read_off, np.int64)
    start = np.asarray(csr.iv_start, np.int64)
    key, rev = np.empty(csr.n_intervals, np.int64), np.empty(csr.n_intervals, np.uint8)
    seen, copies = set(), []
    for r in range(csr.n_reads):
        s = start[off[r]:off[r + 1]]
        h = (s * 7919) % 1009 * 8192 + s                                   # distinct: the starts are
        key[off[r]:off[r + 1]] = np.argsort(np.argsort(h))                 # a function of the read's content
        rev[off[r]:off[r + 1]] = (s * 31 % 7) < 3
        if tuple(s.tolist()) in seen:
            copies.append(r)
        seen.add(tuple(s.tolist()))
    assert len(copies) == 40
    lab = np.zeros(csr.n_reads, np.int32)
    plain = check(idx, lab, key.astype(np.int32), rev)
    k2, r2 = jr.reverse_complement(off, key, rev, copies)
    same_rows(device_rows(idx.ctx, k2.astype(np.int32), r2, loci=False), plain)
    assert (plain['n_obs'] % 2 == 0).all() and (plain['n_reads'] % 2 == 0).all()


# ------------------------------------------------------------------ 2. sort and reduce seams
def chain_cluster(n_loci, hops):
    """One cluster on ``n_loci`` loci 1000 apart: read i holds an interval in locus i and one in each locus
    (i * 7 + 3 * h) % n_loci, so every locus exists and most rows have one observation."""
    reads = []
    for i in range(n_loci):
        at = [i] + [(i * 7 + 3 * h) % n_loci for h in range(1, hops + 1)]
        reads.append([(0, 1000 * a + 3 * t, 1000 * a + 50 + i % 5) for t, a in enumerate(at)])
    return reads


def index_of(ctx, reads):
    chrom, start, end, read = [], [], [], []
    for k, ivs in enumerate(sorted(reads, key=lambda r: min(s for _, s, _ in r))):
        for c, s, e in ivs:
            chrom.append(c), start.append(s), end.append(e), read.append(k)
    return cluster.build_interval_trees(sr.make_data(chrom, start, end, qcode=read), ctx=ctx)


@pytest.mark.parametrize('n_loci', [63, 64, 65, 127, 128, 129])
def test_sort_bit_seams(ctx, n_loci):
    """An end is locus * 2 + side < 2 R and the sort runs on 2 * ceil(log2(2 R)) bits: R loci with 2 R just below,
    at and just above a power of two (2 R is even, so 2^k - 2, 2^k, 2^k + 2).  The last locus's right end, the
    largest end there is, is in a key."""
    idx = index_of(ctx, chain_cluster(n_loci, 2))
    rng = np.random.default_rng(n_loci)
    n = idx.csr.n_intervals
    rev = rng.integers(0, 2, n).astype(np.uint8)
    want = check(idx, np.zeros(idx.csr.n_reads, np.int32), keys_of(idx.csr, 'random', rng), rev)
    loci = lr.loci_of_csr(idx.csr, np.zeros(idx.csr.n_reads, np.int32))
    assert len(loci['start']) == n_loci
    assert (want['locus_b'] * 2 + want['side_b']).max() == 2 * n_loci - 1
    assert (want['n_obs'] == 1).sum() > n_loci                                 # many one-observation rows


@pytest.mark.parametrize('sizes', [(B - 1, B, B + 1, 2 * B + 1), (B, B, 2 * B), (1, B - 1, 1, B + 1, 1)])
def test_one_junction_observed_by_many_reads(ctx, sizes):
    """Cluster k: ``sizes[k]`` reads that all join the same two loci, with their own breakpoints; the segments
    of the sorted observations straddle the reduce kernels' blocks, or end exactly on a block boundary ((B, B,
    2 B): every segment starts and ends on one)."""
    rng = np.random.default_rng(sum(sizes))
    reads, groups = [], []
    for k, n in enumerate(sizes):
        base = 100000 * k
        members = []
        for _ in range(max(n, 2)):                                            # a cluster has two reads at least
            d = int(rng.integers(0, 400))
            members.append(len(reads))
            reads.append([(0, base + d, base + 1000 + d), (1, base + 5000 + d, base + 6000 + 2 * d)])
        if n == 1:                                                            # its second read observes nothing
            reads[-1] = reads[-1][:1]
        groups.append(members)
    idx = index_of(ctx, reads)
    lab = np.arange(len(reads), dtype=np.int32)
    csr = idx.csr
    # membership by position: the read of rank r lies in window floor(start / 100000)
    first = np.asarray(csr.iv_start)[np.asarray(csr.read_off[:-1], np.int64)] // 100000
    for k in range(len(sizes)):
        m = np.flatnonzero(first == k)
        lab[m] = m.min()
    rev = np.zeros(csr.n_intervals, np.uint8)
    want = check(idx, lab, keys_of(csr, 'ascending', rng), rev)
    assert want['n_obs'].tolist() == list(sizes) and want['n_reads'].tolist() == list(sizes)
    assert (want['bp_a_max'] - want['bp_a_min']).max() > 300                   # the extrema come from many elements
    same_rows(device_rows(idx.ctx, keys_of(csr, 'ascending', rng), None, loci=False), want)    # NULL rev = zeros


def test_a_read_observes_one_junction_many_times(ctx):
    """Reads of 64 intervals that go back and forth between two loci: n_obs 63 per read, n_reads 1 per read."""
    reads = []
    for r in range(5):
        reads.append([(0, 100 + r + 2 * t, 400 + t) if t % 2 == 0 else (0, 9000 + r + 2 * t, 9500 + t) for t in range(64)])
    idx = index_of(ctx, reads)
    csr = idx.csr
    # query order = the order the intervals were made in: even t in the first locus ascending, odd t in the second
    off = np.asarray(csr.read_off, np.int64)
    key = np.empty(csr.n_intervals, np.int32)
    for r in range(5):
        s = np.asarray(csr.iv_start[off[r]:off[r + 1]], np.int64)
        t = np.where(s < 9000, (s - 100) // 2, (s - 9000) // 2)               # t + r // 2: the order of t
        key[off[r]:off[r + 1]] = t
    want = check(idx, np.zeros(5, np.int32), key, None)
    assert int(want['n_obs'].sum()) == 5 * 63 and want['n_reads'].max() == 5 and len(want['n_obs']) == 2


# ------------------------------------------------------------------ 3. cluster and locus shapes
def test_clusters_of_one_interval_reads_and_no_clusters(ctx):
    idx = build(ctx, [1] * 40 + [5] * 3, seed=2)
    n = idx.csr.n_reads
    key = keys_of(idx.csr, 'ascending', None)
    lab = groups_of(n, 4, alone=range(40, 43))                               # the longer reads are alone
    got = device_rows(idx.ctx, key, None, lab)
    assert got['off'].tolist() == [0] * 11 and all(got[c].size == 0 for c in jr.COLUMNS)
    same_rows(got, jr.junctions_of_csr(idx.csr, lab, key))
    got = device_rows(idx.ctx, key, None, np.arange(n, dtype=np.int32))      # no clusters
    assert got['off'].tolist() == [0] and all(got[c].size == 0 for c in jr.COLUMNS)


def test_reads_alone_between_clustered_ones_and_65_chromosomes(ctx):
    rng = np.random.default_rng(65)
    lens = [int(x) for x in rng.integers(1, 12, 600)]
    idx = build(ctx, lens, seed=65, n_chroms=65)
    assert idx.csr.n_chroms == 65
    lab = groups_of(len(lens), 6, rng, alone=range(0, len(lens), 3))
    want = check(idx, lab, keys_of(idx.csr, 'random', rng), rng.integers(0, 2, idx.csr.n_intervals).astype(np.uint8))
    loci = lr.loci_of_csr(idx.csr, lab)
    assert len(set(loci['chrom'][want['locus_a']].tolist())) > 50


def test_interval_starting_at_its_locus_end(ctx):
    """start == the locus's end belongs to the locus (end-inclusive); start == end + 1 opens the next one."""
    reads = [[(0, 100, 200), (0, 200, 300), (0, 301, 400)],                   # loci [100, 300] and [301, 400]
             [(0, 150, 160), (0, 300, 300), (0, 400, 450)]]                   # 300 in the first, 400 in the second
    idx = index_of(ctx, reads)
    want = check(idx, np.zeros(2, np.int32), keys_of(idx.csr, 'ascending', None), None)
    # read 0: 0R -> 0L (bp 200 | 200), 0R -> 1L (300 | 301); read 1: 0R -> 0L (160 | 300), 0R -> 1L (300 | 400)
    assert list(zip(want['locus_a'].tolist(), want['side_a'].tolist(), want['locus_b'].tolist(), want['side_b'].tolist(),
                    want['n_obs'].tolist())) == [(0, 0, 0, 1, 2), (0, 1, 1, 0, 2)]
    assert (want['bp_a_min'].tolist(), want['bp_a_max'].tolist()) == ([200, 300], [300, 300])
    assert (want['bp_b_min'].tolist(), want['bp_b_max'].tolist()) == ([160, 301], [200, 400])


# ------------------------------------------------------------------ 4. protocol
def get_rows(c, n_clusters, capacity, fill=-7):
    off = np.full(n_clusters + 1, fill, np.int64)
    cols = [np.full(max(capacity, 1), fill, np.int32) for _ in range(4)]
    sides, bp = np.full(max(capacity, 1), 249, np.uint8), np.full(4 * max(capacity, 1), fill, np.int32)
    p = _lib._ptr
    rc = c._L.fslr_get_cluster_junctions(c._h, p(off), p(cols[0]), p(cols[1]), p(sides), p(cols[2]), p(cols[3]), p(bp),
                                         capacity)
    return rc, off, cols, sides, bp


def untouched(off, cols, sides, bp):
    return (off == -7).all() and all((x == -7).all() for x in cols) and (sides == 249).all() and (bp == -7).all()


def resident_equals(c, want):
    nc, nr = want['off'].size - 1, len(want['n_obs'])
    rc, off, cols, sides, bp = get_rows(c, nc, nr)
    assert rc == _lib.FSLR_OK
    bp = bp.reshape(4, -1)
    got = {'off': off, 'locus_a': cols[0], 'side_a': sides & 1, 'locus_b': cols[1], 'side_b': sides >> 1,
           'n_obs': cols[2], 'n_reads': cols[3], 'bp_a_min': bp[0], 'bp_a_max': bp[1], 'bp_b_min': bp[2], 'bp_b_max': bp[3]}
    same_rows(got, want)


def test_state_and_argument_errors_keep_the_previous_rows():
    c = _lib.Context(0)
    try:
        key0 = np.zeros(4, np.int32)
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*no reads'):
            c.cluster_junctions(key0)
        assert get_rows(c, 0, 0)[0] == _lib.FSLR_ERR_STATE
        rng = np.random.default_rng(3)
        lens = [int(x) for x in rng.integers(1, 9, 300)]
        idx = build(c, lens, seed=9)
        csr, n = idx.csr, idx.csr.n_reads
        key, rev = keys_of(csr, 'random', rng), rng.integers(0, 2, csr.n_intervals).astype(np.uint8)
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*no cluster table'):
            c.cluster_junctions(key, rev)
        lab = groups_of(n, 5, rng)
        c.cluster_table(lab)
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_loci first'):
            c.cluster_junctions(key, rev)
        want = check(idx, lab, key, rev)
        nc, nr = want['off'].size - 1, len(want['n_obs'])
        assert nr > 100
        with pytest.raises(_lib.FslrError, match=STATE):
            c.cluster_junctions_timings()                           # not a profiling context
        # short capacity: nothing is written
        rc, *outs = get_rows(c, nc, nr - 1)
        assert rc == _lib.FSLR_ERR_INVALID and untouched(*outs) and 'capacity' in c._L.fslr_last_error(c._h).decode()
        # NULL outputs are skipped
        n_obs = np.empty(nr, np.int32)
        assert c._L.fslr_get_cluster_junctions(c._h, None, None, None, None, _lib._ptr(n_obs), None, None, nr) == _lib.FSLR_OK
        np.testing.assert_array_equal(n_obs, want['n_obs'])
        # wrong n_intervals, NULL keys
        with pytest.raises(_lib.FslrError, match=f'{INVALID}.*n_intervals'):
            c.cluster_junctions(key[:-1], rev[:-1])
        nrows = _lib.ctypes.c_int64(-7)
        assert c._L.fslr_cluster_junctions(c._h, None, _lib._ptr(rev), csr.n_intervals, _lib.ctypes.byref(nrows)) == \
            _lib.FSLR_ERR_INVALID
        assert nrows.value == -7 and 'NULL' in c._L.fslr_last_error(c._h).decode()
        resident_equals(c, want)
        # the loci rows and the table are as they were
        same = c.cluster_loci_rows()
        for a, b in zip(same, c.cluster_loci()):
            np.testing.assert_array_equal(a, b)
        # that cluster_loci dropped the junction rows (they name the rows it replaced)
        assert get_rows(c, nc, nr)[0] == _lib.FSLR_ERR_STATE
        same_rows(device_rows(c, key, rev, loci=False), want)
        # reads again without an index: refused, the rows still answer
        c.load_csr(csr, np.zeros(csr.n_intervals, np.int32))
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_build_index'):
            c.cluster_junctions(key, rev)
        resident_equals(c, want)
        c.build_index()
        # a new table drops the loci rows and the junction rows with them
        c.cluster_table(lab)
        assert get_rows(c, nc, nr)[0] == _lib.FSLR_ERR_STATE
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_loci first'):
            c.cluster_junctions(key, rev)
        same_rows(device_rows(c, key, rev), want)
    finally:
        c.close()


def test_two_runs_give_the_same_bytes_and_the_timings_call():
    c = _lib.Context(0, profiling=True)
    try:
        rng = np.random.default_rng(8)
        lens = [int(x) for x in rng.integers(1, 17, 2000)]
        idx = build(c, lens, seed=8)
        key, rev = keys_of(idx.csr, 'random', rng), rng.integers(0, 2, idx.csr.n_intervals).astype(np.uint8)
        lab = groups_of(len(lens), 7, rng, alone=range(0, len(lens), 5))
        runs = [device_rows(c, key, rev, lab)]
        assert c.cluster_junctions_timings()['junctions'] > 0
        runs.append(device_rows(c, key, rev, loci=False))
        same_rows(runs[0], jr.junctions_of_csr(idx.csr, lab, key, rev))
        assert [runs[0][k].tobytes() for k in runs[0]] == [runs[1][k].tobytes() for k in runs[0]]
    finally:
        c.close()


def test_append_and_remove_leave_a_stale_table():
    data, csr, cid, nc, kw = fixture_membership('cfg1_1k_x3')
    codes = np.unique(data.qcode)
    late = np.isin(data.qcode, codes[codes.size * 2 // 3:])
    idx = cluster.build_interval_trees(data.select(~late))
    try:
        c = idx.ctx
        first = idx.cluster_junctions(np.arange(idx.csr.n_intervals), None, query(idx, idx.data, kw))
        assert len(first) > 0
        idx.append(data.select(late))
        key = np.zeros(idx.csr.n_intervals, np.int32)
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_table again'):
            c.cluster_junctions(key)
        n_obs = np.empty(len(first), np.int32)                       # the rows made before still answer
        assert c._L.fslr_get_cluster_junctions(c._h, None, None, None, None, _lib._ptr(n_obs), None, None, len(first)) == \
            _lib.FSLR_OK
        np.testing.assert_array_equal(n_obs, first.n_obs)
        lab = np.zeros(idx.csr.n_reads, np.int32)
        check(idx, lab, key)
        keep = np.ones(idx.csr.n_reads, bool)
        keep[::7] = False
        idx.remove(keep=keep)
        key = np.zeros(idx.csr.n_intervals, np.int32)
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_table again'):
            c.cluster_junctions(key)
        lab = np.zeros(idx.csr.n_reads, np.int32)
        check(idx, lab, key)
    finally:
        idx.ctx.close()


def test_virtual_reads_are_refused():
    data, csr, cid, nc, kw = fixture_membership('longreads_400')
    idx = cluster.build_interval_trees(data)
    try:
        assert idx.long is not None
        lab = np.arange(idx.csr.n_reads, dtype=np.int32)
        lab[:2] = 0
        idx.ctx.cluster_table(lab)
        idx.ctx.cluster_loci()
        with pytest.raises(_lib.FslrError, match=f'{INVALID}.*more than 64'):
            idx.ctx.cluster_junctions(np.zeros(idx.ctx.n_intervals, np.int32))
        with pytest.raises(NotImplementedError, match='more than 64'):
            idx.cluster_junctions(np.zeros(idx.csr.n_intervals, np.int32))
    finally:
        idx.ctx.close()


def test_multi_gpu_index_refuses():
    mg = cluster.MultiGpuIndex(sr.make_data([1, 1], [0, 5], [9, 9]), 2)
    with pytest.raises(NotImplementedError, match='n_gpus=1'):
        mg.cluster_junctions([0, 1])


# ------------------------------------------------------------------ 5. the wrapper and the command line
def bed_inputs(name, data):
    """qstart and '+' / '-' of the data list's rows, and the rev bits the CLI derives (main.junction_inputs' rule,
    restated with loops)."""
    bed = fx.input_bed(name)
    rows = np.asarray(data.index, np.int64)
    primary = {}
    for q, s, seq in zip(bed['qname'].tolist(), bed['strand'].tolist(), bed['seq'].tolist()):
        if isinstance(seq, str) and seq and q not in primary:
            primary[q] = s == '-'
    rev = np.asarray([(s == '-') != primary.get(q, False) for q, s in zip(bed['qname'].tolist(), bed['strand'].tolist())])
    return bed['qstart'].to_numpy()[rows], bed['strand'].to_numpy()[rows], rev[rows].astype(np.uint8)


def test_wrapper_on_a_golden_fixture():
    name = 'cfg1_1k_x3'
    data, csr, cid, nc, kw = fixture_membership(name)
    qstart, strand, _ = bed_inputs(name, data)
    pos = np.asarray(csr.data_pos, np.int64)
    want = jr.junctions(csr.read_off, csr.iv_chrom, csr.iv_start, csr.iv_end, cid, nc, qstart[pos], strand[pos] == '-')
    idx = cluster.build_interval_trees(data)
    try:
        got = idx.cluster_junctions(qstart, strand, query(idx, data, kw))     # makes the table and the loci rows
        assert isinstance(got, cluster.ClusterJunctions) and len(got) == len(want['n_obs']) > 0
        same_rows({k: getattr(got, k) for k in ('off',) + jr.COLUMNS}, want)
        same_rows({k: getattr(idx.cluster_junctions(qstart, strand == '-'), k) for k in ('off',) + jr.COLUMNS}, want)
        loci = lr.loci(csr.read_off, csr.iv_chrom, csr.iv_start, csr.iv_end, cid, nc)
        np.testing.assert_array_equal(got.loci.start, loci['start'])
        frame = got.to_frame()
        assert list(frame.columns) == ['cluster', 'chrom_a', 'side_a', 'locus_a', 'bp_a_min', 'bp_a_max', 'chrom_b',
                                       'side_b', 'locus_b', 'bp_b_min', 'bp_b_max', 'n_obs', 'n_reads']
        np.testing.assert_array_equal(frame['cluster'], np.repeat(np.arange(nc), np.diff(want['off'])))
        np.testing.assert_array_equal(idx._dense_chroms(frame['chrom_b'].to_numpy()), loci['chrom'][want['locus_b']])
        with pytest.raises(ValueError, match='intervals'):
            idx.cluster_junctions(qstart[:-1])
    finally:
        idx.ctx.close()


def test_cli_cluster_junctions_in_both_io_modes(tmp_path):
    name = 'cfg1_1k_x3'
    data, csr, cid, nc, kw = fixture_membership(name)
    qstart, _, rev = bed_inputs(name, data)
    idx = cluster.build_interval_trees(data)
    try:
        frame = idx.cluster_junctions(qstart, rev, query(idx, data, kw)).to_frame()
    finally:
        idx.ctx.close()
    from fslr_amd import fastcli
    name_of = {v: k for k, v in fastcli.chrom_map(list(pd.unique(fx.input_bed(name)['chrom']))).items()}
    for col in ('chrom_a', 'chrom_b'):
        frame[col] = [name_of[c] for c in frame[col].tolist()]
    want = frame.to_csv(sep='\t', index=False)
    texts = {}
    for io_flag, more in (('--native-io', ()), ('--pandas-io', ()), ('--native-io', ('--cluster-loci',))):
        tmp = tmp_path / (io_flag.strip('-') + str(len(more)))
        tmp.mkdir()
        res = run_cli(name, str(tmp), io_flag, '--cluster-junctions', *more)
        assert res.exit_code == 0, (res.output, res.exception)
        texts[(io_flag, more)] = open(os.path.join(str(tmp), 'fx.mappings.cluster_junctions.bed')).read()
        for which in ('cluster', 'representative'):
            assert open(os.path.join(str(tmp), f'fx.mappings.{which}.bed')).read() == fx.expected_text(name, which), which
        assert os.path.exists(os.path.join(str(tmp), 'fx.mappings.cluster_loci.bed')) == bool(more)
    assert len(set(texts.values())) == 1 and want.count('\n') > 10
    assert texts[('--native-io', ())] == want


def test_cli_long_reads_print_a_notice_and_write_no_file(tmp_path):
    res = run_cli('longreads_400', str(tmp_path), '--cluster-junctions')
    assert res.exit_code == 0, (res.output, res.exception)
    assert 'more than 64 intervals' in res.output
    assert not os.path.exists(os.path.join(str(tmp_path), 'fx.mappings.cluster_junctions.bed'))


def test_cli_refuses_several_gpus(tmp_path):
    res = run_cli('cfg1_1k_x3', str(tmp_path), '--cluster-junctions', '--gpus=2')
    assert res.exit_code == 2 and '--gpus 1' in res.output
    assert sorted(os.listdir(str(tmp_path))) == ['fx.bwa_dodi.bam', 'fx.mappings.bed']
