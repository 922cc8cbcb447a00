"""Cluster paths on the device (fslr_cluster_paths, fslr_get_cluster_paths) against tests/paths_ref.py, which
tests/test_paths_ref.py pins to hand-worked cases.  Clusters come from host label vectors, so read lengths, lane
groups, row counts and group sizes are exact; the query keys and strand bits are made per CSR interval.  Every
comparison is exact, dtypes included."""
import os

import numpy as np
import pandas as pd
import pytest

import fixtures as fx
import junctions_ref as jr
import loci_ref as lr
import paths_ref as pr
import search_ref as sr
from fslr_amd import _lib, cluster
from test_gpu_junctions import bed_inputs, build, groups_of, index_of, keys_of
from test_gpu_loci import fixture_membership, query, run_cli

pytestmark = pytest.mark.gpu

INVALID = f'fslr error {_lib.FSLR_ERR_INVALID}'
STATE = f'fslr error {_lib.FSLR_ERR_STATE}'
B = 256                        # the kernels' block: groups of B + 1 and 2 B + 1 reads straddle blocks


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def device(c, qkey, rev=None, labels=None, loci=True):
    if labels is not None:
        c.cluster_table(labels)
    if loci:
        c.cluster_loci()
    return dict(zip(pr.NAMES, c.cluster_paths(qkey, rev)))


def same(got, want, names=pr.NAMES):
    for k in names:
        assert got[k].dtype == want[k].dtype, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def check(idx, labels, qkey, rev=None):
    want = pr.paths_of_csr(idx.csr, labels, qkey, rev)
    same(device(idx.ctx, qkey, rev, labels), want)
    # the n_reads of a cluster's rows sum to the cluster's size
    cid, nc = lr.cids_of_labels(labels)
    sums = np.add.reduceat(np.append(want['n_reads'], 0).astype(np.int64), want['off'][:-1]) if nc else np.zeros(0, np.int64)
    np.testing.assert_array_equal(sums, np.bincount(cid[cid >= 0], minlength=nc))
    return want


def index_with(ctx, reads):
    """reads: lists of (chrom, start, end, key, rev) with all starts distinct.  The index and (qkey, rev) per CSR
    interval."""
    idx = index_of(ctx, [[(c, s, e) for c, s, e, _, _ in r] for r in reads])
    by = {s: (k, v) for r in reads for _, s, _, k, v in r}
    assert len(by) == idx.csr.n_intervals
    kv = np.asarray([by[s] for s in np.asarray(idx.csr.iv_start).tolist()], np.int64)
    return idx, kv[:, 0].astype(np.int32), kv[:, 1].astype(np.uint8)


# ------------------------------------------------------------------ 1. lane groups and chains
SEAM_LENS = (1, 2, 15, 16, 17, 32, 33, 63, 64)


@pytest.mark.parametrize('mode', ['ascending', 'descending', 'random', 'equal', 'extreme'])
def test_read_lengths_alone_in_a_wavefront(ctx, mode):
    """Each seam length with three one-interval reads behind it: the long read decides its wavefront's group width
    alone."""
    lens = [x for n in SEAM_LENS for x in (n, 1, 1, 1)] * 2
    idx = build(ctx, lens, seed=len(mode), share=4)
    rng = np.random.default_rng(1)
    want = check(idx, groups_of(len(lens), 8), keys_of(idx.csr, mode, rng), rng.integers(0, 2, idx.csr.n_intervals).astype(np.uint8))
    assert sorted(set(np.diff(want['tok_off']).tolist())) == sorted(SEAM_LENS)
    assert int(want['n_reads'].sum()) == len(lens) and want['flipped'].any() and not want['flipped'].all()


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
    assert (want['path_of_read'] == -1).sum() >= len(lens) // 9 and len(want['n_reads']) > 80


# ------------------------------------------------------------------ 2. grouping seams
@pytest.mark.parametrize('copies', [2, 3])
def test_every_read_twice_or_three_times_and_reverse_complemented(ctx, copies):
    """A cluster that holds every read ``copies`` times: n_reads is a multiple of it and first_read the lowest rank.
    With the second copy of each read from the other strand (order reversed, strand bits flipped) the rows and
    path_of_read are the same bytes; flipped changes for exactly those reads whose path is no palindrome."""
    rng = np.random.default_rng(4)
    reads = []
    for r in range(40):
        n = int(rng.integers(1, 20))
        reads.append([(int(rng.integers(0, 2)), int(s), int(s) + int(rng.integers(0, 300))) for s in
                      rng.choice(6000, n, replace=False)])
    idx = index_of(ctx, reads * copies)
    csr = idx.csr
    off, start = np.asarray(csr.read_off, np.int64), np.asarray(csr.iv_start, np.int64)
    key, rev = np.empty(csr.n_intervals, np.int64), np.empty(csr.n_intervals, np.uint8)
    seen, second = {}, []
    for r in range(csr.n_reads):
        s = start[off[r]:off[r + 1]]
        h = (s * 7919) % 1009 * 8192 + s                                   # distinct: the starts are
        key[off[r]:off[r + 1]] = np.argsort(np.argsort(h))                 # a function of the read's content
        rev[off[r]:off[r + 1]] = (s * 31 % 7) < 3
        t = tuple(s.tolist())
        seen[t] = seen.get(t, 0) + 1
        if seen[t] == 2:
            second.append(r)
    assert len(second) == 40
    lab = np.zeros(csr.n_reads, np.int32)
    plain = check(idx, lab, key.astype(np.int32), rev)
    assert (plain['n_reads'] % copies == 0).all() and (plain['n_reads'] == copies).any()
    np.testing.assert_array_equal(plain['first_read'], [np.flatnonzero(plain['path_of_read'] == i)[0] for i in range(len(plain['n_reads']))])
    k2, r2 = jr.reverse_complement(off, key, rev, second)
    turned = device(idx.ctx, k2.astype(np.int32), r2, loci=False)
    same(turned, plain, pr.NAMES[:-1])
    rows = pr.rows_of(plain)
    pal = np.asarray([rows[p][0] == tuple(t ^ 1 for t in reversed(rows[p][0])) for p in plain['path_of_read']])
    np.testing.assert_array_equal(turned['flipped'] != plain['flipped'], np.isin(np.arange(csr.n_reads), second) & ~pal)
    assert (turned['flipped'] != plain['flipped']).sum() > 30


def seam_chains(length=24, n_loci=8):
    """One cluster on ``n_loci`` loci 100000 apart (chromosome 0): a base chain of ``length`` pieces, every proper
    prefix of it, and for every position d a chain that differs from the base there and nowhere else.  A chain
    starts at locus 0 forward (token 0) and goes on in loci >= 2, so it is canonical as it stands (the other
    direction starts with a token >= 4) and the first difference of two chains lies where it was put; the chain
    that differs at position 0 starts at locus 1 forward (token 2).  Reads as (chrom, start, end, key, rev), the
    starts distinct, the key the chain position."""
    base = [(0, 0)] + [(2 + (i * 5) % (n_loci - 2), (i * 7 % 3) == 0) for i in range(1, length)]
    chains = [base] + [base[:k] for k in range(1, length)]
    for d in range(length):
        other = list(base)
        other[d] = (1, 0) if d == 0 else (2 + (base[d][0] - 1) % (n_loci - 2), base[d][1]) if d % 2 else (base[d][0], not base[d][1])
        chains.append(other)
    return [[(0, 100000 * a + 64 * k + i, 100000 * a + 99000, i, int(v)) for i, (a, v) in enumerate(ch)]
            for k, ch in enumerate(chains)]


def test_prefixes_and_first_differences_at_every_position_under_every_pack(ctx, monkeypatch):
    """Chains that are proper prefixes of one another and chains that first differ at position 0, at the last
    position and at every position between, so at every boundary between two sort keys, with one, two, three and
    the default number of tokens per key.  The bytes are the same under all four."""
    idx, qkey, rev = index_with(ctx, seam_chains())
    lab = np.zeros(idx.csr.n_reads, np.int32)
    want = pr.paths_of_csr(idx.csr, lab, qkey, rev)
    assert not want['flipped'].any() and (want['n_reads'] == 1).all() and len(want['n_reads']) == 48
    assert sorted(np.diff(want['tok_off']).tolist()) == list(range(1, 24)) + [24] * 25
    idx.ctx.cluster_table(lab)
    idx.ctx.cluster_loci()
    blobs = []
    for pack in ('1', '2', '3', None):
        if pack is None:
            monkeypatch.delenv('FSLR_PATHS_PACK', raising=False)
        else:
            monkeypatch.setenv('FSLR_PATHS_PACK', pack)
        got = device(idx.ctx, qkey, rev, loci=False)
        same(got, want)
        blobs.append([got[k].tobytes() for k in pr.NAMES])
    assert all(b == blobs[0] for b in blobs)


@pytest.mark.parametrize('sizes', [(B + 1, 2 * B + 1), (B, 2 * B, 1)])
def test_one_path_shared_by_many_reads(ctx, sizes):
    """Cluster k: ``sizes[k]`` reads that all walk the same two loci (and one more read of one interval): the
    groups of the final order straddle the 256-thread blocks or end exactly on their boundaries."""
    rng = np.random.default_rng(sum(sizes))
    reads = []
    for k, n in enumerate(sizes):
        base = 100000 * k
        for _ in range(n):
            d = int(rng.integers(0, 400))
            reads.append([(0, base + d, base + 1000 + d), (1, base + 5000 + d, base + 6000 + 2 * d)])
        reads.append([(0, base + 500, base + 600)])
    idx = index_of(ctx, reads)
    csr = idx.csr
    first = np.asarray(csr.iv_start)[np.asarray(csr.read_off[:-1], np.int64)] // 100000
    lab = np.arange(len(reads), dtype=np.int32)
    for k in range(len(sizes)):
        m = np.flatnonzero(first == k)
        lab[m] = m.min()
    want = check(idx, lab, keys_of(csr, 'ascending', None), None)
    assert want['n_reads'].tolist() == [x for n in sizes for x in (1, n)]
    assert want['off'].tolist() == list(range(0, 2 * len(sizes) + 1, 2))


def test_a_cluster_whose_reads_all_differ_and_300_clusters_of_two(ctx):
    n = 300
    reads = [[(0, 1000 * i + 1, 1000 * i + 50), (0, 1000 * ((i + 1) % n) + 2 + (i + 1 == n), 1000 * ((i + 1) % n) + 60)]
             for i in range(n)]
    idx = index_of(ctx, reads)
    csr = idx.csr
    key = (np.asarray(csr.iv_start) % 1000).astype(np.int32)               # the first piece, then the second
    want = check(idx, np.zeros(n, np.int32), key, None)
    assert len(want['n_reads']) == n and (want['n_reads'] == 1).all()
    rng = np.random.default_rng(2)
    lens = [int(x) for x in rng.integers(1, 7, 2 * n)]
    idx = build(ctx, lens, seed=6, share=2)
    want = check(idx, groups_of(2 * n, 2), keys_of(idx.csr, 'random', rng), rng.integers(0, 2, idx.csr.n_intervals).astype(np.uint8))
    assert want['off'].size == n + 1 and (np.diff(want['off']) >= 1).all() and (np.diff(want['off']) == 1).any()


def test_palindromic_chains_of_two_and_four(ctx):
    reads = [[(0, 100, 200, 0, 0), (0, 150, 250, 1, 1)], [(0, 120, 130, 0, 0)],                    # a:+ a:-
             [(0, 100100, 100200, 0, 0), (0, 101000, 101100, 1, 0), (0, 101010, 101090, 2, 1),     # a:+ b:+ b:- a:-
              (0, 100110, 100190, 3, 1)], [(0, 100120, 100130, 0, 1)]]
    idx, qkey, rev = index_with(ctx, reads)
    want = check(idx, np.asarray([0, 0, 2, 2], np.int32), qkey, rev)
    assert [t for t, _, _ in pr.rows_of(want)] == [(0,), (0, 1), (2,), (2, 4, 5, 3)]
    assert want['flipped'].tolist() == [0, 0, 0, 1]


# ------------------------------------------------------------------ 3. protocol
def get_rows(c, n_clusters, n_reads, row_capacity, token_capacity, fill=-7):
    wide = [np.full(n_clusters + 1, fill, np.int64), np.full(max(row_capacity, 0) + 1, fill, np.int64)]
    ints = [np.full(max(k, 1), fill, np.int32) for k in (row_capacity, row_capacity, token_capacity, n_reads)]
    byts = [np.full(max(k, 1), 249, np.uint8) for k in (token_capacity, n_reads)]
    p = _lib._ptr
    rc = c._L.fslr_get_cluster_paths(c._h, p(wide[0]), p(wide[1]), p(ints[0]), p(ints[1]), p(ints[2]), p(byts[0]),
                                     p(ints[3]), p(byts[1]), row_capacity, token_capacity)
    return rc, wide, ints, byts


def untouched(wide, ints, byts):
    return all((x == -7).all() for x in wide + ints) and all((x == 249).all() for x in byts)


def resident_equals(c, want):
    nc, nr, nt, n = want['off'].size - 1, len(want['n_reads']), len(want['locus']), len(want['flipped'])
    rc, wide, ints, byts = get_rows(c, nc, n, nr, nt)
    assert rc == _lib.FSLR_OK
    got = {'off': wide[0], 'tok_off': wide[1], 'n_reads': ints[0][:nr], 'first_read': ints[1][:nr], 'locus': ints[2][:nt],
           'rev': byts[0][:nt], 'path_of_read': ints[3][:n], 'flipped': byts[1][:n]}
    same(got, want)


def test_state_and_argument_errors_keep_the_previous_rows():
    c = _lib.Context(0)
    try:
        key0 = np.zeros(4, np.int32)
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*no reads'):
            c.cluster_paths(key0)
        assert get_rows(c, 0, 0, 0, 0)[0] == _lib.FSLR_ERR_STATE
        rng = np.random.default_rng(3)
        lens = [int(x) for x in rng.integers(1, 9, 300)]
        idx = build(c, lens, seed=9)
        csr, n = idx.csr, idx.csr.n_reads
        key, rev = keys_of(csr, 'random', rng), rng.integers(0, 2, csr.n_intervals).astype(np.uint8)
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*no cluster table'):
            c.cluster_paths(key, rev)
        lab = groups_of(n, 5, rng)
        c.cluster_table(lab)
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_loci first'):
            c.cluster_paths(key, rev)
        want = check(idx, lab, key, rev)
        nc, nr, nt = want['off'].size - 1, len(want['n_reads']), len(want['locus'])
        assert nr > 100 and nt > nr
        with pytest.raises(_lib.FslrError, match=STATE):
            c.cluster_paths_timings()                               # not a profiling context
        # a capacity one too small, rows or tokens: nothing is written
        for rcap, tcap in ((nr - 1, nt), (nr, nt - 1)):
            rc, *outs = get_rows(c, nc, n, rcap, tcap)
            assert rc == _lib.FSLR_ERR_INVALID and untouched(*outs) and 'capacity' in c._L.fslr_last_error(c._h).decode()
        # NULL outputs are skipped
        n_reads = np.empty(nr, np.int32)
        assert c._L.fslr_get_cluster_paths(c._h, None, None, _lib._ptr(n_reads), None, None, None, None, None, nr, nt) == _lib.FSLR_OK
        np.testing.assert_array_equal(n_reads, want['n_reads'])
        # wrong n_intervals, NULL keys
        with pytest.raises(_lib.FslrError, match=f'{INVALID}.*n_intervals'):
            c.cluster_paths(key[:-1], rev[:-1])
        cnt = _lib.ctypes.c_int64(-7)
        assert c._L.fslr_cluster_paths(c._h, None, _lib._ptr(rev), csr.n_intervals, _lib.ctypes.byref(cnt), None) == \
            _lib.FSLR_ERR_INVALID
        assert cnt.value == -7 and 'NULL' in c._L.fslr_last_error(c._h).decode()
        resident_equals(c, want)
        # the junction rows survive a paths call and the path rows a junctions call
        junctions = c.cluster_junctions(key, rev)
        resident_equals(c, want)
        same(device(c, key, rev, loci=False), want)
        n_obs = np.empty(len(junctions[5]), np.int32)
        assert c._L.fslr_get_cluster_junctions(c._h, None, None, None, None, _lib._ptr(n_obs), None, None, n_obs.size) == _lib.FSLR_OK
        np.testing.assert_array_equal(n_obs, junctions[5])
        # the loci rows are as they were; making them again drops the path rows (they name the rows it replaced)
        for a, b in zip(c.cluster_loci_rows(), c.cluster_loci()):
            np.testing.assert_array_equal(a, b)
        assert get_rows(c, nc, n, nr, nt)[0] == _lib.FSLR_ERR_STATE
        same(device(c, key, rev, loci=False), want)
        # reads again without an index: refused, the rows still answer
        c.load_csr(csr, np.zeros(csr.n_intervals, np.int32))
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_build_index'):
            c.cluster_paths(key, rev)
        resident_equals(c, want)
        c.build_index()
        # a new table drops the loci rows and the path rows with them
        c.cluster_table(lab)
        assert get_rows(c, nc, n, nr, nt)[0] == _lib.FSLR_ERR_STATE
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_loci first'):
            c.cluster_paths(key, rev)
        same(device(c, key, rev), want)
        # no clusters: no rows, off all zero, every read -1
        got = device(c, key, rev, np.arange(n, dtype=np.int32))
        assert got['off'].tolist() == [0] and got['tok_off'].tolist() == [0] and got['n_reads'].size == 0
        assert (got['path_of_read'] == -1).all() and not got['flipped'].any()
        same(got, pr.paths_of_csr(csr, np.arange(n, dtype=np.int32), key, rev))
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
        runs = [device(c, key, rev, lab)]
        assert c.cluster_paths_timings()['paths'] > 0
        runs.append(device(c, key, rev, loci=False))
        same(runs[0], pr.paths_of_csr(idx.csr, lab, key, rev))
        assert [runs[0][k].tobytes() for k in pr.NAMES] == [runs[1][k].tobytes() for k in pr.NAMES]
    finally:
        c.close()


def test_append_leaves_a_stale_table():
    data, csr, cid, nc, kw = fixture_membership('cfg1_1k_x3')
    codes = np.unique(data.qcode)
    late = np.isin(data.qcode, codes[codes.size * 2 // 3:])
    idx = cluster.build_interval_trees(data.select(~late))
    try:
        c = idx.ctx
        first = idx.cluster_paths(np.arange(idx.csr.n_intervals), None, query(idx, idx.data, kw))
        assert len(first) > 0
        idx.append(data.select(late))
        key = np.zeros(idx.csr.n_intervals, np.int32)
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_table again'):
            c.cluster_paths(key)
        n_reads = np.empty(len(first), np.int32)                     # the rows made before still answer
        assert c._L.fslr_get_cluster_paths(c._h, None, None, _lib._ptr(n_reads), None, None, None, None, None, len(first),
                                           len(first.locus)) == _lib.FSLR_OK
        np.testing.assert_array_equal(n_reads, first.n_reads)
        check(idx, np.zeros(idx.csr.n_reads, np.int32), key)
    finally:
        idx.ctx.close()


def test_virtual_reads_and_a_multi_gpu_index_are_refused():
    data, csr, cid, nc, kw = fixture_membership('longreads_400')
    idx = cluster.build_interval_trees(data)
    try:
        assert idx.long is not None
        lab = np.arange(idx.csr.n_reads, dtype=np.int32)
        lab[:2] = 0
        idx.ctx.cluster_table(lab)
        idx.ctx.cluster_loci()
        with pytest.raises(_lib.FslrError, match=f'{INVALID}.*more than 64'):
            idx.ctx.cluster_paths(np.zeros(idx.ctx.n_intervals, np.int32))
        with pytest.raises(NotImplementedError, match='more than 64'):
            idx.cluster_paths(np.zeros(idx.csr.n_intervals, np.int32))
    finally:
        idx.ctx.close()
    mg = cluster.MultiGpuIndex(sr.make_data([1, 1], [0, 5], [9, 9]), 2)
    with pytest.raises(NotImplementedError, match='n_gpus=1'):
        mg.cluster_paths([0, 1])


# ------------------------------------------------------------------ 4. the wrapper and the command line
def expected_frame(name):
    """to_frame()'s rows for a golden fixture from the plain statement alone, chromosomes as names."""
    from fslr_amd import fastcli
    data, csr, cid, nc, kw = fixture_membership(name)
    qstart, _, rev = bed_inputs(name, data)
    pos = np.asarray(csr.data_pos, np.int64)
    loci = lr.loci(csr.read_off, csr.iv_chrom, csr.iv_start, csr.iv_end, cid, nc)
    want = pr.paths(csr.read_off, csr.iv_chrom, csr.iv_start, csr.iv_end, cid, nc, qstart[pos], rev[pos], loci)
    name_of = {v: k for k, v in fastcli.chrom_map(list(pd.unique(fx.input_bed(name)['chrom']))).items()}
    dense_names = [name_of[v] for v in np.unique(data.chrom).tolist()]
    names = np.asarray(data.qnames, dtype=object)[np.asarray(csr.read_qcode)]
    rows = []
    for c in range(nc):
        for i in range(int(want['off'][c]), int(want['off'][c + 1])):
            a, b = int(want['tok_off'][i]), int(want['tok_off'][i + 1])
            pieces = [f"{dense_names[loci['chrom'][k]]}:{loci['start'][k]}-{loci['end'][k]}:{'-' if v else '+'}"
                      for k, v in zip(want['locus'][a:b].tolist(), want['rev'][a:b].tolist())]
            rows.append((c, i - int(want['off'][c]), int(want['n_reads'][i]), b - a, names[want['first_read'][i]], ','.join(pieces)))
    return want, rows, (data, kw, qstart, rev)


def test_wrapper_and_cli_on_a_golden_fixture(tmp_path):
    name = 'cfg1_1k_x3'
    want, rows, (data, kw, qstart, rev) = expected_frame(name)
    assert len(rows) > 10
    idx = cluster.build_interval_trees(data)
    try:
        got = idx.cluster_paths(qstart, rev, query(idx, data, kw))           # makes the table and the loci rows
        assert isinstance(got, cluster.ClusterPaths) and len(got) == len(rows)
        same({k: getattr(got, k) for k in pr.NAMES}, want)
        frame = got.to_frame()
        assert list(frame.columns) == ['cluster', 'path', 'n_reads', 'n_loci', 'first_read', 'structure']
        assert frame[['cluster', 'path', 'n_reads', 'n_loci', 'first_read']].values.tolist() == [list(r[:5]) for r in rows]
        rf = got.read_frame()
        assert list(rf.columns) == ['qname', 'cluster', 'path', 'flipped'] and len(rf) == idx.csr.n_reads
        np.testing.assert_array_equal(rf['cluster'].to_numpy() >= 0, want['path_of_read'] >= 0)
        dom = got.dominant()
        assert dom.shape == (want['off'].size - 1,)
        assert all(want['n_reads'][d] == want['n_reads'][a:b].max() for d, a, b in zip(dom, want['off'][:-1], want['off'][1:]))
        with pytest.raises(ValueError, match='intervals'):
            idx.cluster_paths(qstart[:-1])
    finally:
        idx.ctx.close()
    res = run_cli(name, str(tmp_path), '--cluster-paths')
    assert res.exit_code == 0, (res.output, res.exception)
    text = open(os.path.join(str(tmp_path), 'fx.mappings.cluster_paths.bed')).read()
    assert text == 'cluster\tpath\tn_reads\tn_loci\tfirst_read\tstructure\n' + ''.join('\t'.join(map(str, r)) + '\n' for r in rows)
    for which in ('cluster', 'representative'):
        assert open(os.path.join(str(tmp_path), f'fx.mappings.{which}.bed')).read() == fx.expected_text(name, which), which


def test_cli_long_reads_print_a_notice_and_several_gpus_are_refused(tmp_path):
    a, b = tmp_path / 'a', tmp_path / 'b'
    a.mkdir(), b.mkdir()
    res = run_cli('longreads_400', str(a), '--cluster-paths')
    assert res.exit_code == 0, (res.output, res.exception)
    assert 'more than 64 intervals' in res.output and 'file is written' in res.output
    assert not os.path.exists(os.path.join(str(a), 'fx.mappings.cluster_paths.bed'))
    res = run_cli('cfg1_1k_x3', str(b), '--cluster-paths', '--gpus=2')
    assert res.exit_code == 2 and '--gpus 1' in res.output
    assert sorted(os.listdir(str(b))) == ['fx.bwa_dodi.bam', 'fx.mappings.bed']
