"""Path segments on the device (fslr_cluster_path_segments, fslr_get_cluster_path_segments) against
tests/segments_ref.py, which tests/test_segments_ref.py pins to hand-worked cases.  Clusters come from host label
vectors, so read lengths, lane groups and the reads per path (the k of the selection tiers) are exact.  Every
comparison is exact, dtypes included.

A reference coordinate is below 2^30 (the upload refuses more), so the extreme starts and ends are 0 and 2^30 - 1;
the query columns and the gaps take the whole int32 range."""
import os

import numpy as np
import pandas as pd
import pytest

import fixtures as fx
import loci_ref as lr
import paths_ref as pr
import search_ref as sr
import segments_ref as sg
from fslr_amd import _lib, cluster, synth
from fslr_amd.prep import fold_overlap_threshold, pass_table
from test_gpu_junctions import bed_inputs, build, groups_of, index_of, keys_of
from test_gpu_loci import fixture_membership, query, run_cli

pytestmark = pytest.mark.gpu

INVALID = f'fslr error {_lib.FSLR_ERR_INVALID}'
STATE = f'fslr error {_lib.FSLR_ERR_STATE}'
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
COORD_MAX = (1 << 30) - 1


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def device(c, qkey, qend=None, rev=None, labels=None, loci=True, paths=True):
    if labels is not None:
        c.cluster_table(labels)
    if loci:
        c.cluster_loci()
    if paths:
        c.cluster_paths(qkey, rev)
    return dict(zip(sg.NAMES, c.cluster_path_segments(qkey, qend)))


def same(got, want):
    for k in sg.NAMES:
        assert got[k].dtype == want[k].dtype == np.int32, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def blob(got):
    return [got[k].tobytes() for k in sg.NAMES]


def check(idx, labels, qkey, qend=None, rev=None):
    p, want = sg.segments_of_csr(idx.csr, labels, qkey, qend, rev)
    same(device(idx.ctx, qkey, qend, rev, labels), want)
    last = np.asarray(p['tok_off'][1:], np.int64) - 1                     # the last slot of every row holds no gap
    assert not any(want[k][last].any() for k in sg.NAMES[6:])
    return p, want


def ends_of(qkey, rng, mode='random'):
    if mode == 'extreme':
        return rng.choice(np.asarray([I32_MIN, -1, 0, I32_MAX], np.int64), qkey.size).astype(np.int32)
    return (qkey.astype(np.int64) + rng.integers(-30, 30, qkey.size)).astype(np.int32)


# ------------------------------------------------------------------ 1. emit and flipping
SEAM_LENS = (1, 2, 15, 16, 17, 32, 33, 63, 64)


@pytest.mark.parametrize('mode', ['ascending', 'descending', 'random', 'equal', 'extreme'])
def test_read_lengths_alone_in_a_wavefront(ctx, mode):
    """Each seam length with three one-interval reads behind it, so the long read decides its wavefront's group
    width alone."""
    lens = [x for n in SEAM_LENS for x in (n, 1, 1, 1)]
    idx = build(ctx, lens, seed=len(mode), share=4)
    rng = np.random.default_rng(1)
    key = keys_of(idx.csr, mode, rng)
    rev = rng.integers(0, 2, idx.csr.n_intervals).astype(np.uint8)
    p, want = check(idx, groups_of(len(lens), 8), key, ends_of(key, rng, mode), rev)
    assert sorted(set(np.diff(p['tok_off']).tolist())) == sorted(SEAM_LENS)
    assert p['flipped'].any() and not p['flipped'].all()
    if mode == 'extreme':
        assert (want['gap_min'] == I32_MIN).any() and (want['gap_max'] == I32_MAX).any()


def test_read_lengths_mixed_four_to_a_wavefront(ctx):
    """Quads that keep 16-lane groups, quads one read pushes to 32 or 64 lanes, one-interval reads between them and
    a last quad that is not full; three copies of the list, the copies of a read in one cluster."""
    rng = np.random.default_rng(11)
    quads = [(2, 15, 16, 3), (16, 16, 16, 16), (17, 2, 2, 2), (5, 32, 1, 16), (33, 16, 2, 1), (2, 3, 63, 4),
             (64, 64, 64, 64), (1, 1, 1, 1), (64, 1, 33, 17), (16, 17, 32, 33), (9, 2)]
    lens = [n for q in quads for n in q] * 3
    idx = build(ctx, lens, seed=3)
    key = keys_of(idx.csr, 'random', rng)
    lab = groups_of(len(lens), 5, rng, alone=range(4, len(lens), 9))
    p, _ = check(idx, lab, key, ends_of(key, rng), rng.integers(0, 2, idx.csr.n_intervals).astype(np.uint8))
    assert (p['path_of_read'] == -1).sum() >= len(lens) // 9 and len(p['n_reads']) > 80


def test_every_read_twice_and_reverse_complemented(ctx):
    """A cluster that holds every read twice: every row has an even number of reads.  With the second copy of each
    read from the other strand (query coordinates mirrored, strand bits flipped) the segment bytes are the same:
    a reversed read puts its pieces in the path's slots and its gaps on the same links."""
    rng = np.random.default_rng(4)
    reads = []
    for r in range(60):
        n = int(rng.integers(1, 65))
        reads.append([(int(rng.integers(0, 2)), int(s), int(s) + int(rng.integers(0, 300))) for s in
                      rng.choice(6000000, n, replace=False)])
    idx = index_of(ctx, reads * 2)
    csr = idx.csr
    off, start = np.asarray(csr.read_off, np.int64), np.asarray(csr.iv_start, np.int64)
    qs, qe, rev = (np.empty(csr.n_intervals, np.int64) for _ in range(3))
    seen, second = {}, []
    for r in range(csr.n_reads):
        s = start[off[r]:off[r + 1]]
        h = (s * 7919) % 1009 * 8192 + s                                   # distinct: the starts are
        rank = np.argsort(np.argsort(h))                                   # a function of the read's content
        qs[off[r]:off[r + 1]] = 100 * rank + s % 20
        qe[off[r]:off[r + 1]] = 100 * rank + s % 20 + 80 + (s // 20) % 20  # gaps in [-18, 39]; the ends ascend too
        rev[off[r]:off[r + 1]] = (s * 31 % 7) < 3
        t = tuple(s.tolist())
        seen[t] = seen.get(t, 0) + 1
        if seen[t] == 2:
            second.append(r)
    assert len(second) == 60
    lab = np.zeros(csr.n_reads, np.int32)
    p, plain = check(idx, lab, qs.astype(np.int32), qe.astype(np.int32), rev.astype(np.uint8))
    assert (p['n_reads'] % 2 == 0).all() and (plain['gap_min'] < 0).any() and (plain['gap_max'] > 0).any()
    # (a palindromic path keeps a reversed read's own order: none here, the loci are far apart)
    assert not any(t == tuple(x ^ 1 for x in reversed(t)) for t, _, _ in pr.rows_of(p))
    # the same molecule from the other strand: query position x of a molecule of length Q becomes Q - x
    q2, e2, r2 = qs.copy(), qe.copy(), rev.copy().astype(np.uint8)
    for r in second:
        s = slice(int(off[r]), int(off[r + 1]))
        q2[s], e2[s], r2[s] = 10000 - qe[s], 10000 - qs[s], r2[s] ^ 1
    turned = device(idx.ctx, q2.astype(np.int32), e2.astype(np.int32), r2, loci=False)
    same(turned, plain)
    assert blob(turned) == blob(plain)
    same(turned, sg.segments_of_csr(csr, lab, q2, e2, r2)[1])


# ------------------------------------------------------------------ 2. the selection tiers
def one_path_cluster(ctx, k, order, rng, pieces=2):
    """k reads that walk the same ``pieces`` loci (chromosome 0, then 1): the intervals of a chromosome share a
    position (1000; 5000 for the distinct values), so each chromosome is one locus.  The values per ``order``; the
    first piece's query key is below the second's in every read.  Returns (idx, qkey, qend)."""
    def values():
        if order == 'equal':
            return np.full(k, 5), np.full(k, 2000)
        if order == 'distinct':
            return rng.permutation(k), 5000 + rng.permutation(k) * 3
        if order == 'extreme':
            return rng.choice([0, 999], k), rng.choice([1001, COORD_MAX], k)
        return rng.integers(0, 50, k), 1000 + rng.integers(0, 50, k)
    cols = [values() for _ in range(pieces)]
    reads = [[(c, int(cols[c][0][i]), int(cols[c][1][i])) for c in range(pieces)] for i in range(k)]
    idx = index_of(ctx, reads)
    second = np.asarray(idx.csr.iv_chrom) == 1
    n = idx.csr.n_intervals
    if order == 'extreme':
        qkey = np.where(second, rng.choice([-2, I32_MAX], n), I32_MIN)
        qend = rng.choice([I32_MIN, -1, I32_MAX], n)
    elif order == 'equal':
        qkey, qend = np.where(second, 100, 0), np.full(n, 90)
    else:
        qkey = np.where(second, 1000 + rng.integers(0, 40, n), rng.integers(0, 40, n))
        qend = qkey + (rng.permutation(n) if order == 'distinct' else rng.integers(900, 1100, n))
    return idx, qkey.astype(np.int32), qend.astype(np.int32)


@pytest.mark.parametrize('k', [1, 2, 16, 17, 32, 33, 64, 65, 255, 256, 257, 4096, 4097])
def test_selection_seams_at_the_defaults(ctx, k):
    """One cluster of k reads on one path, k on both sides of every lane-group width and tier boundary (64 | 65,
    4096 | 4097), with equal values, all distinct ones, the extremes and random ones with ties."""
    rng = np.random.default_rng(k)
    for order in ('equal', 'distinct', 'extreme', 'random'):
        # the largest two: one-interval reads, and one two-interval case
        pieces = 2 if k < 4096 or order == 'distinct' else 1
        idx, qkey, qend = one_path_cluster(ctx, k, order, rng, pieces)
        lab = np.zeros(k, np.int32)
        if k == 1:                                             # a cluster needs two reads: a second path of one read
            idx = index_of(ctx, [[(0, 5, 2000), (1, 5, 2000)], [(0, 9000, 9001)]])
            qkey, qend, lab = np.asarray([0, 100, 0], np.int32), np.asarray([90, 190, 7], np.int32), np.zeros(2, np.int32)
        p, want = check(idx, lab, qkey, qend)
        assert p['n_reads'].max() == max(k, 1) and len(want['start_med']) == (3 if k == 1 else pieces)
        if order == 'extreme' and pieces == 2 and k >= 64:       # (5/6)^64: some read has each extreme gap
            assert want['gap_min'][0] == I32_MIN and want['gap_max'][0] == I32_MAX
            assert want['start_min'][0] == 0 and want['end_max'][0] == COORD_MAX


def test_moved_seams_give_the_same_bytes(ctx, monkeypatch):
    """Clusters of 1, 2, 3, 5, 8, 9, 16, 17 and 70 reads on one path each: under (FSLR_SEGS_SMALL, FSLR_SEGS_LDS) =
    (64, 4096) all sit in the lane-group tier or the LDS tier, under (1, 2), (4, 8) and (16, 16) they move through
    the LDS and the select tier.  The bytes are the same."""
    rng = np.random.default_rng(21)
    sizes = (1, 2, 3, 5, 8, 9, 16, 17, 70)
    reads, lab = [], []
    for g, k in enumerate(sizes):
        base = 100000 * g
        for _ in range(k):
            d = int(rng.integers(0, 400))
            reads.append([(0, base + d, base + 1000 + d), (1, base + 5000 + d, base + 6000 + 2 * d), (0, base + 20000 + d, base + 21000)])
        reads.append([(0, base + 500, base + 600)])
    idx = index_of(ctx, reads)
    csr = idx.csr
    first = np.asarray(csr.iv_start)[np.asarray(csr.read_off[:-1], np.int64)] // 100000
    lab = np.arange(len(reads), dtype=np.int32)
    for g in range(len(sizes)):
        m = np.flatnonzero(first == g)
        lab[m] = m.min()
    qkey = keys_of(csr, 'ascending', None)
    qend = ends_of(qkey, rng)
    p, want = sg.segments_of_csr(csr, lab, qkey, qend)
    assert sorted(p['n_reads'].tolist()) == sorted([1] * len(sizes) + [k for k in sizes if k > 1] + [1])
    idx.ctx.cluster_table(lab)
    idx.ctx.cluster_loci()
    idx.ctx.cluster_paths(qkey)
    blobs = []
    for small, lds in ((None, None), ('1', '2'), ('4', '8'), ('16', '16')):
        for name, v in (('FSLR_SEGS_SMALL', small), ('FSLR_SEGS_LDS', lds)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, v)
        got = device(idx.ctx, qkey, qend, loci=False, paths=False)
        same(got, want)
        blobs.append(blob(got))
    assert all(b == blobs[0] for b in blobs)


# ------------------------------------------------------------------ 3. the shape of the rows
def test_several_paths_per_cluster_and_unclustered_reads(ctx):
    rng = np.random.default_rng(5)
    # 450 reads, each twice (the copies take neighbouring ranks): clusters of six ranks hold three paths of two reads,
    # or of one where a copy is left alone
    reads = [[(int(rng.integers(0, 3)), 10000 * i + int(s), 10000 * i + int(s) + int(rng.integers(1, 300)))
              for s in rng.choice(9000, int(rng.integers(1, 7)), replace=False)] for i in range(450)]
    idx = index_of(ctx, reads * 2)
    start = np.asarray(idx.csr.iv_start, np.int64)
    key = (start * 7919 % 1009).astype(np.int32)                        # functions of the start: the same in both copies
    lab = groups_of(900, 6, None, alone=range(0, 900, 7))
    p, want = check(idx, lab, key, ends_of(key, rng), (start * 31 % 7 < 3).astype(np.uint8))
    assert (np.diff(p['off']) > 1).any() and (p['path_of_read'] == -1).any() and (p['n_reads'] > 1).any()
    # without qend: the same starts and ends, every gap 0
    got = device(idx.ctx, key, None, loci=False, paths=False)
    for k in sg.NAMES[:6]:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert not any(got[k].any() for k in sg.NAMES[6:]) and any(want[k].any() for k in sg.NAMES[6:])


def test_clusters_whose_rows_all_hold_one_read_and_no_clusters_at_all(ctx):
    n = 300
    reads = [[(0, 1000 * i + 1, 1000 * i + 50), (0, 1000 * ((i + 1) % n) + 2 + (i + 1 == n), 1000 * ((i + 1) % n) + 60)]
             for i in range(n)]
    idx = index_of(ctx, reads)
    key = (np.asarray(idx.csr.iv_start) % 1000).astype(np.int32)
    rng = np.random.default_rng(2)
    p, want = check(idx, np.zeros(n, np.int32), key, ends_of(key, rng))
    assert (p['n_reads'] == 1).all() and len(p['n_reads']) == n
    np.testing.assert_array_equal(want['start_min'], want['start_max'])
    # no clusters at all: zero tokens, and the getter succeeds
    got = device(idx.ctx, key, ends_of(key, rng), None, np.arange(n, dtype=np.int32))
    assert all(got[k].shape == (0,) and got[k].dtype == np.int32 for k in sg.NAMES)
    assert idx.ctx._L.fslr_get_cluster_path_segments(idx.ctx._h, None, None, None, 0) == _lib.FSLR_OK


# ------------------------------------------------------------------ 4. protocol
def get_rows(c, token_capacity, fill=-7):
    outs = [np.full(3 * max(token_capacity, 1), fill, np.int32) for _ in range(3)]
    p = _lib._ptr
    return c._L.fslr_get_cluster_path_segments(c._h, p(outs[0]), p(outs[1]), p(outs[2]), token_capacity), outs


def resident_equals(c, want):
    nt = len(want['start_min'])
    rc, outs = get_rows(c, nt)
    assert rc == _lib.FSLR_OK
    got = {f'{kind}_{w}': o[i * nt:(i + 1) * nt] for kind, o in zip(('start', 'end', 'gap'), outs)
           for i, w in enumerate(('min', 'med', 'max'))}
    same(got, want)


def test_state_and_argument_errors_keep_the_previous_rows():
    c = _lib.Context(0)
    try:
        key0 = np.zeros(4, np.int32)
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*no reads'):
            c.cluster_path_segments(key0)
        assert get_rows(c, 0)[0] == _lib.FSLR_ERR_STATE
        rng = np.random.default_rng(3)
        lens = [int(x) for x in rng.integers(1, 9, 300)]
        idx = build(c, lens, seed=9)
        csr, n = idx.csr, idx.csr.n_reads
        key, rev = keys_of(csr, 'random', rng), rng.integers(0, 2, csr.n_intervals).astype(np.uint8)
        qend = ends_of(key, rng)
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*no cluster table'):
            c.cluster_path_segments(key, qend)
        lab = groups_of(n, 5, rng)
        c.cluster_table(lab)
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_loci first'):
            c.cluster_path_segments(key, qend)
        c.cluster_loci()
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_paths first'):
            c.cluster_path_segments(key, qend)
        p, want = check(idx, lab, key, qend, rev)
        nt = len(want['start_min'])
        assert nt > 300
        with pytest.raises(_lib.FslrError, match=STATE):
            c.cluster_path_segments_timings()                       # not a profiling context
        # a capacity one too small: nothing is written
        rc, outs = get_rows(c, nt - 1)
        assert rc == _lib.FSLR_ERR_INVALID and all((o == -7).all() for o in outs)
        assert 'capacity' in c._L.fslr_last_error(c._h).decode()
        # NULL outputs are skipped
        gap = np.empty((3, nt), np.int32)
        assert c._L.fslr_get_cluster_path_segments(c._h, None, None, _lib._ptr(gap), nt) == _lib.FSLR_OK
        np.testing.assert_array_equal(gap[1], want['gap_med'])
        # wrong n_intervals, NULL keys: refused, the rows stay
        with pytest.raises(_lib.FslrError, match=f'{INVALID}.*n_intervals'):
            c.cluster_path_segments(key[:-1], qend[:-1])
        cnt = _lib.ctypes.c_int64(-7)
        assert c._L.fslr_cluster_path_segments(c._h, None, _lib._ptr(qend), csr.n_intervals, _lib.ctypes.byref(cnt)) == \
            _lib.FSLR_ERR_INVALID
        assert cnt.value == -7 and 'NULL' in c._L.fslr_last_error(c._h).decode()
        resident_equals(c, want)
        # another column than the paths': no error, and the contract's answer for that column's order
        other = keys_of(csr, 'descending', None)
        got = dict(zip(sg.NAMES, c.cluster_path_segments(other, qend)))
        same(got, sg.segments(csr.read_off, csr.iv_start, csr.iv_end, p, other, qend))
        same(device(c, key, qend, rev, loci=False, paths=False), want)
        # the path, junction and loci rows are left alone
        paths_before = c.cluster_paths(key, rev)
        assert get_rows(c, nt)[0] == _lib.FSLR_ERR_STATE           # a successful paths call drops the segment rows
        same(device(c, key, qend, rev, loci=False, paths=False), want)
        n_reads = np.empty(len(paths_before[2]), np.int32)
        assert c._L.fslr_get_cluster_paths(c._h, None, None, _lib._ptr(n_reads), None, None, None, None, None,
                                           n_reads.size, nt) == _lib.FSLR_OK
        np.testing.assert_array_equal(n_reads, paths_before[2])
        # cluster_loci drops the path rows and the segment rows with them
        c.cluster_loci()
        assert get_rows(c, nt)[0] == _lib.FSLR_ERR_STATE
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_paths first'):
            c.cluster_path_segments(key, qend)
        same(device(c, key, qend, rev, loci=False), want)
        # reads again without an index: refused, the rows still answer
        c.load_csr(csr, np.zeros(csr.n_intervals, np.int32))
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_build_index'):
            c.cluster_path_segments(key, qend)
        resident_equals(c, want)
        c.build_index()
        # a new table drops them
        c.cluster_table(lab)
        assert get_rows(c, nt)[0] == _lib.FSLR_ERR_STATE
        same(device(c, key, qend, rev), want)
    finally:
        c.close()


def test_two_runs_give_the_same_bytes_and_the_timings_call():
    c = _lib.Context(0, profiling=True)
    try:
        rng = np.random.default_rng(8)
        lens = [int(x) for x in rng.integers(1, 17, 2000)]
        idx = build(c, lens, seed=8)
        key, rev = keys_of(idx.csr, 'random', rng), rng.integers(0, 2, idx.csr.n_intervals).astype(np.uint8)
        qend = ends_of(key, rng)
        lab = groups_of(len(lens), 7, rng, alone=range(0, len(lens), 5))
        runs = [device(c, key, qend, rev, lab)]
        assert c.cluster_path_segments_timings()['segments'] > 0
        runs.append(device(c, key, qend, rev, loci=False, paths=False))
        same(runs[0], sg.segments_of_csr(idx.csr, lab, key, qend, rev)[1])
        assert blob(runs[0]) == blob(runs[1])
    finally:
        c.close()


def test_append_leaves_a_stale_table():
    data, csr, cid, nc, kw = fixture_membership('cfg1_1k_x3')
    codes = np.unique(data.qcode)
    late = np.isin(data.qcode, codes[codes.size * 2 // 3:])
    idx = cluster.build_interval_trees(data.select(~late))
    try:
        c = idx.ctx
        first = idx.cluster_path_segments(np.arange(idx.csr.n_intervals), None, None, query(idx, idx.data, kw))
        assert len(first) > 0
        idx.append(data.select(late))
        key = np.zeros(idx.csr.n_intervals, np.int32)
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_table again'):
            c.cluster_path_segments(key)
        assert get_rows(c, len(first))[0] == _lib.FSLR_OK            # the rows made before still answer
        keep = np.ones(idx.csr.n_reads, bool)
        keep[:3] = False
        idx.remove(keep)
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_table again'):
            c.cluster_path_segments(np.zeros(idx.csr.n_intervals, np.int32))
        check(idx, np.zeros(idx.csr.n_reads, np.int32), np.zeros(idx.csr.n_intervals, np.int32))
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
        key = np.zeros(idx.csr.n_intervals, np.int32)
        idx.ctx.cluster_paths_any(key)
        with pytest.raises(_lib.FslrError, match=f'{INVALID}.*more than 64'):
            idx.ctx.cluster_path_segments(key)
        with pytest.raises(NotImplementedError, match='more than 64'):
            idx.cluster_path_segments(key)
    finally:
        idx.ctx.close()
    mg = cluster.MultiGpuIndex(sr.make_data([1, 1], [0, 5], [9, 9]), 2)
    with pytest.raises(NotImplementedError, match='n_gpus=1'):
        mg.cluster_path_segments([0, 1])


# ------------------------------------------------------------------ 5. end to end
def test_synthetic_reads_clustered_by_the_query():
    csr = synth.generate(2000, 16, 11).interval_data().csr()
    c = _lib.Context(0)
    try:
        c.load_csr(csr, fold_overlap_threshold(csr.iv_aln, 0.8))
        c.reserve_edges(max(1 << 16, 12 * csr.n_reads))
        c.build_index()
        c.run_query(0.96, 0.75, pass_table([1, 1, 0.66, 0.66, 0.66, 0.5]), 10)
        c.apply_edge_cap(10)
        c.components()
        labels = c.labels()
        c.cluster_table()
        rng = np.random.default_rng(12)
        key = keys_of(csr, 'random', rng)
        qend, rev = ends_of(key, rng), rng.integers(0, 2, csr.n_intervals).astype(np.uint8)
        p, want = sg.segments_of_csr(csr, labels, key, qend, rev)
        assert len(want['start_med']) > 200 and (p['n_reads'] > 1).any()
        same(device(c, key, qend, rev), want)
    finally:
        c.close()


def expected_lines(name):
    """The file's lines for a golden fixture from the plain statement alone, chromosomes as names."""
    from fslr_amd import fastcli
    data, csr, cid, nc, kw = fixture_membership(name)
    qstart, _, rev = bed_inputs(name, data)
    qend = fx.input_bed(name)['qend'].to_numpy()[np.asarray(data.index, np.int64)]
    pos = np.asarray(csr.data_pos, np.int64)
    loci = lr.loci(csr.read_off, csr.iv_chrom, csr.iv_start, csr.iv_end, cid, nc)
    p = pr.paths(csr.read_off, csr.iv_chrom, csr.iv_start, csr.iv_end, cid, nc, qstart[pos], rev[pos], loci)
    want = sg.segments(csr.read_off, csr.iv_start, csr.iv_end, p, qstart[pos], qend[pos])
    name_of = {v: k for k, v in fastcli.chrom_map(list(pd.unique(fx.input_bed(name)['chrom']))).items()}
    dense_names = [name_of[v] for v in np.unique(data.chrom).tolist()]
    lines = []
    for c in range(nc):
        for i in range(int(p['off'][c]), int(p['off'][c + 1])):
            for j, s in enumerate(range(int(p['tok_off'][i]), int(p['tok_off'][i + 1]))):
                lines.append((dense_names[loci['chrom'][p['locus'][s]]], want['start_med'][s], want['end_med'][s], c,
                              i - int(p['off'][c]), j, '-' if p['rev'][s] else '+', p['n_reads'][i], want['start_min'][s],
                              want['start_max'][s], want['end_min'][s], want['end_max'][s], want['gap_min'][s],
                              want['gap_med'][s], want['gap_max'][s]))
    return p, want, lines, (data, kw, qstart, qend, rev)


HEADER = 'chrom\tstart\tend\tcluster\tpath\tpiece\tstrand\tn_reads\tstart_min\tstart_max\tend_min\tend_max\tgap_min\tgap\tgap_max\n'


def test_wrapper_and_cli_on_a_golden_fixture(tmp_path):
    name = 'cfg1_1k_x3'
    p, want, lines, (data, kw, qstart, qend, rev) = expected_lines(name)
    assert len(lines) > 10 and (want['start_min'] < want['start_max']).any()
    idx = cluster.build_interval_trees(data)
    try:
        got = idx.cluster_path_segments(qstart, qend, rev, query(idx, data, kw))       # makes the table, loci and paths
        assert isinstance(got, cluster.ClusterPathSegments) and len(got) == len(lines)
        same(dict(zip(sg.NAMES, got.columns())), want)
        np.testing.assert_array_equal(got.paths.tok_off, p['tok_off'])
        again = idx.cluster_path_segments(qstart, qend, rev)                           # on the resident path rows
        assert again.paths is got.paths
        same(dict(zip(sg.NAMES, again.columns())), want)
        idx.cluster_loci()                                                             # drops them: made again
        third = idx.cluster_path_segments(qstart, None, rev)
        assert third.paths is not got.paths and not third.gap_med.any()
        np.testing.assert_array_equal(third.start_med, want['start_med'])
        frame = got.to_frame()
        assert frame[['cluster', 'path', 'piece', 'start', 'end', 'gap']].values.tolist() == \
            [[r[3], r[4], r[5], r[1], r[2], r[13]] for r in lines]
        assert got.structure(0).split(',')[0].endswith(f":{want['start_med'][0]}-{want['end_med'][0]}:{'-' if p['rev'][0] else '+'}")
        with pytest.raises(ValueError, match='intervals'):
            idx.cluster_path_segments(qstart, qend[:-1])
    finally:
        idx.ctx.close()
    text = HEADER + ''.join('\t'.join(map(str, r)) + '\n' for r in lines)
    for io_flag in ('--native-io', '--pandas-io'):
        out = tmp_path / io_flag.strip('-')
        out.mkdir()
        res = run_cli(name, str(out), io_flag, '--cluster-path-segments')
        assert res.exit_code == 0, (res.output, res.exception)
        assert open(os.path.join(str(out), 'fx.mappings.cluster_path_segments.bed')).read() == text
        for which in ('cluster', 'representative'):
            assert open(os.path.join(str(out), f'fx.mappings.{which}.bed')).read() == fx.expected_text(name, which), which
    # with --cluster-paths before it (its rows are reused) the same bytes
    out = tmp_path / 'both'
    out.mkdir()
    res = run_cli(name, str(out), '--cluster-paths', '--cluster-path-segments')
    assert res.exit_code == 0, (res.output, res.exception)
    assert open(os.path.join(str(out), 'fx.mappings.cluster_path_segments.bed')).read() == text


def test_cli_long_reads_print_a_notice_and_several_gpus_are_refused(tmp_path):
    a, b = tmp_path / 'a', tmp_path / 'b'
    a.mkdir(), b.mkdir()
    res = run_cli('longreads_400', str(a), '--cluster-path-segments', '--cluster-long-reads')
    assert res.exit_code == 0, (res.output, res.exception)
    assert 'more than 64 intervals' in res.output and 'file is written' in res.output
    assert not os.path.exists(os.path.join(str(a), 'fx.mappings.cluster_path_segments.bed'))
    res = run_cli('cfg1_1k_x3', str(b), '--cluster-path-segments', '--gpus=2')
    assert res.exit_code == 2 and '--gpus 1' in res.output
    assert sorted(os.listdir(str(b))) == ['fx.bwa_dodi.bam', 'fx.mappings.bed']
