"""Cluster loci on the device (fslr_cluster_loci, fslr_get_cluster_loci) against tests/loci_ref.py, which
tests/test_loci_ref.py pins to hand-worked cases and a coverage statement.  Cluster composition is chosen
freely through host label vectors, so the inputs sit on the scan's seams: T is the scan's tile, set to its
smallest value through FSLR_LOCI_TILE.  Every comparison is exact."""
import io
import os
import shutil

import numpy as np
import pandas as pd
import pytest

import fixtures as fx
import loci_ref as lr
import search_ref as sr
from fslr_amd import _lib, cluster, fastcli

pytestmark = pytest.mark.gpu

INVALID = f'fslr error {_lib.FSLR_ERR_INVALID}'
STATE = f'fslr error {_lib.FSLR_ERR_STATE}'
T = 256                       # the smallest tile: 256 threads x 1 element
BIG = 1 << 29
CUTOFFS = [1, 1, 0.66, 0.66, 0.66, 0.5]


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture
def small_tile(monkeypatch):
    monkeypatch.setenv('FSLR_LOCI_TILE', str(T))


class Builder:
    """Intervals of reads numbered as they are made; clusters as lists of those numbers."""

    def __init__(self, seed=0):
        self.rng = np.random.default_rng(seed)
        self.chrom, self.start, self.end, self.read = [], [], [], []
        self.n_reads, self.groups = 0, []

    def read_of(self, ivs):
        for c, s, e in ivs:
            self.chrom.append(c), self.start.append(s), self.end.append(e), self.read.append(self.n_reads)
        self.n_reads += 1
        return self.n_reads - 1

    def cluster(self, ivs, per_read=37):
        """One cluster whose reads hold ``ivs`` between them (at least two reads, at most per_read each)."""
        ivs = list(ivs)
        k = max(2, -(-len(ivs) // per_read))
        deal = self.rng.permutation(len(ivs)) % k if len(ivs) >= k else np.arange(len(ivs))
        reads = [self.read_of([ivs[i] for i in np.flatnonzero(deal == r)]) for r in range(k) if (deal == r).any()]
        assert len(reads) >= 2
        self.groups.append(reads)
        return reads

    def singles(self, n, n_chroms, span):
        for _ in range(n):
            s = self.rng.integers(0, span, int(self.rng.integers(1, 4)))
            self.read_of([(int(self.rng.integers(0, n_chroms)), int(x), int(x) + int(self.rng.integers(0, span // 4 + 1)))
                          for x in s])

    def index(self, ctx, shuffle_seed=None):
        data = sr.make_data(self.chrom, self.start, self.end, qcode=self.read, shuffle_seed=shuffle_seed)
        return cluster.build_interval_trees(data, ctx=ctx)

    def labels(self, csr):
        code = np.asarray(csr.read_qcode, np.int64)
        rank_of = np.empty(self.n_reads, np.int64)
        rank_of[code] = np.arange(code.size)
        lab = np.arange(code.size, dtype=np.int32)
        for g in self.groups:
            r = rank_of[np.asarray(g)]
            lab[r] = r.min()
        return lab


def device_rows(c, labels=None):
    if labels is not None:
        c.cluster_table(labels)
    off, chrom, start, end, ni, nr = c.cluster_loci()
    return {'off': off, 'chrom': chrom, 'start': start, 'end': end, 'n_intervals': ni, 'n_reads': nr}


def same_rows(got, want):
    for k in ('off',) + lr.COLUMNS:
        assert got[k].dtype == want[k].dtype, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def check(idx, labels):
    want = lr.loci_of_csr(idx.csr, labels)
    same_rows(device_rows(idx.ctx, labels), want)
    return want


def chain(chrom, n, at, rng, step=10, reach=25):
    """n intervals from ``at`` on, starts ``step`` apart on average, some touching, some apart."""
    s = at + np.cumsum(rng.integers(0, 2 * step, n))
    return [(chrom, int(x), int(x) + int(rng.integers(0, reach))) for x in s]


# ------------------------------------------------------------------ 1. segment sizes at the seams
@pytest.mark.parametrize('sizes', [(T - 1, T, T + 1, 2 * T + 1), (63, 64, 65), (1, 2, 64, 3, T, 1, 2 * T)])
def test_segment_sizes(ctx, small_tile, sizes):
    b = Builder(sum(sizes))
    at = 0
    for k, n in enumerate(sizes):
        # every cluster on one chromosome: its segment is its n intervals (n == 1: two chromosomes, one each)
        if n == 1:
            b.groups.append([b.read_of([(0, at, at + 5)]), b.read_of([(1, at, at + 5)])])
        else:
            b.cluster(chain(k % 2, n, at, b.rng))
        b.singles(5, 2, 50 * sum(sizes))
        at += 7
    idx = b.index(ctx)
    want = check(idx, b.labels(idx.csr))
    assert want['off'].size == len(sizes) + 1 and len(want['start']) > len(sizes)


# ------------------------------------------------------------------ 2. the carry is the maximum
@pytest.mark.parametrize('tiles', [3, 300])
def test_one_locus_over_many_tiles(ctx, small_tile, tiles):
    """The first interval's end covers everything behind it: the carry across tiles (300: across every round of
    the carry pass, 256 tiles each) is the running maximum, not the last element's end."""
    rng = np.random.default_rng(tiles)
    n = tiles * T + 17
    ivs = [(0, 5, BIG)] + [(0, 10 + 3 * k, 11 + 3 * k + int(rng.integers(0, 2))) for k in range(n - 3)]
    ivs += [(0, BIG, BIG + 4), (0, BIG + 5, BIG + 6)]         # start == max end merges, max end + 1 does not
    b = Builder(tiles)
    b.cluster(ivs, per_read=61)
    idx = b.index(ctx)
    want = check(idx, b.labels(idx.csr))
    assert list(zip(want['start'].tolist(), want['end'].tolist(), want['n_intervals'].tolist())) == \
        [(5, BIG + 4, n - 1), (BIG + 5, BIG + 6, 1)]


# ------------------------------------------------------------------ 3. the carry does not leak
@pytest.mark.parametrize('n_first', [T, T + T // 2, 2 * T, 64, 65])
@pytest.mark.parametrize('how', ['next_cluster', 'next_chromosome'])
def test_no_leak_behind_a_huge_end(ctx, small_tile, n_first, how):
    """A segment of n_first intervals whose last one ends far away; the next segment (the next cluster on the
    same chromosome, or the same cluster's next chromosome) starts at a tile start or mid-tile with small
    coordinates and several loci of its own."""
    b = Builder(n_first)
    first = [(0, 2 * k, 2 * k + 1) for k in range(n_first - 1)] + [(0, 2 * n_first, BIG)]
    nxt = [(0 if how == 'next_cluster' else 1, 3 + 40 * k, 3 + 40 * k + (k % 3) * 15) for k in range(T + 9)]
    if how == 'next_cluster':
        b.cluster(first)                          # holds the smallest start: rank 0, cluster 0
        b.cluster(nxt)
    else:
        b.cluster(first + nxt)
    idx = b.index(ctx)
    want = check(idx, b.labels(idx.csr))
    sel = slice(int(want['off'][1]), None) if how == 'next_cluster' else want['chrom'] == 1
    assert want['end'][sel].max() < BIG and len(want['end'][sel]) > T // 2


def test_single_interval_segments_everywhere(ctx, small_tile):
    """Two reads of one interval each on different chromosomes per cluster: every position is a segment of its
    own, those at wave and tile starts included."""
    b = Builder(1)
    for k in range(T + 40):
        b.groups.append([b.read_of([(0, 3 * k, 3 * k + 100)]), b.read_of([(1 + k % 2, 3 * k, 3 * k + 100)])])
    idx = b.index(ctx)
    want = check(idx, b.labels(idx.csr))
    assert (want['n_intervals'] == 1).all() and np.diff(want['off']).tolist() == [2] * (T + 40)


def test_many_equal_starts_in_any_order(ctx, small_tile):
    rng = np.random.default_rng(8)
    ivs = [(0, 100, 100 + int(e)) for e in rng.integers(0, 50, 2 * T + 3)] + [(0, 150, 160), (0, 161, 170)] + \
          [(0, 161, 161)] * 70
    rows = []
    for seed in (None, 1, 2):
        b = Builder(3)
        b.cluster(ivs)
        b.singles(40, 1, 300)
        idx = b.index(ctx, shuffle_seed=seed)
        rows.append(check(idx, b.labels(idx.csr)))
    for r in rows[1:]:
        same_rows(r, rows[0])                        # the tie order of equal starts changes nothing


# ------------------------------------------------------------------ 4. random inputs, extremes
def random_index(ctx, seed, n_reads, n_chroms, span, shuffle_seed=None):
    rng = np.random.default_rng(seed)
    b = Builder(seed)
    for _ in range(n_reads):
        k = int(rng.integers(1, 9))
        s = rng.integers(0, span, k)
        b.read_of([(int(rng.integers(0, n_chroms)), int(x), int(x) + int(rng.integers(0, 60))) for x in s])
    return b.index(ctx, shuffle_seed), rng


def random_labels(rng, n, p_single=0.5, n_groups=40):
    g = rng.integers(0, n_groups, n)
    g[rng.random(n) < p_single] = -1
    lab = np.arange(n, dtype=np.int32)
    for k in range(n_groups):
        r = np.flatnonzero(g == k)
        if r.size:
            lab[r] = r.min()
    return lab


@pytest.mark.parametrize('n_chroms', [3, 64, 65, 115])
def test_random_with_reads_alone_everywhere(ctx, small_tile, n_chroms):
    """65 and 115 chromosomes take the index build's other path and the gather's search in global memory."""
    idx, rng = random_index(ctx, n_chroms, 1500, n_chroms, 4000)
    assert idx.csr.n_chroms == n_chroms
    want = check(idx, random_labels(rng, idx.csr.n_reads))
    assert len(set(want['chrom'].tolist())) == n_chroms


def test_all_alone_and_all_together(ctx):
    idx, rng = random_index(ctx, 5, 3000, 4, 20000)
    n = idx.csr.n_reads
    got = device_rows(idx.ctx, np.arange(n, dtype=np.int32))
    assert got['off'].tolist() == [0] and all(got[k].size == 0 for k in lr.COLUMNS)
    want = check(idx, np.zeros(n, np.int32))                       # the default tile
    assert want['off'].tolist() == [0, len(want['start'])] and want['n_intervals'].sum() == idx.csr.n_intervals


# ------------------------------------------------------------------ 5. reads of more than 64 intervals
def test_virtual_reads(ctx, small_tile):
    """A read of 130 intervals and one of exactly 65 in one cluster with short reads (labels over the real
    reads): a locus that holds intervals of two chunks of one read counts the read once, and the loci behind
    interval 64 hold second- and third-chunk intervals only."""
    b = Builder(13)
    long1 = []
    for i in range(130):
        if 60 <= i <= 70:                                         # one chain across the chunk seam at 64
            long1.append((0, 60000 + 50 * (i - 60), 60000 + 50 * (i - 60) + 80))
        else:
            long1.append((i % 3 == 0, 1000 * i, 1000 * i + 100))
    r1 = b.read_of(long1)
    r2 = b.read_of([(0, 1000 * i + 10, 1000 * i + 60) for i in range(65)])
    shorts = [b.read_of([(0, 64000 + 30 * k, 64000 + 30 * k + 40), (1, 99000, 99050 + k)]) for k in range(5)]
    b.groups.append([r1, r2] + shorts)
    b.cluster(chain(0, 90, 500, b.rng))
    b.singles(60, 2, 130000)
    idx = b.index(ctx)
    assert idx.long is not None and sorted(idx.long.tolist())[-2:] == [65, 130]
    lab = b.labels(idx.csr)
    assert lab.size == idx.csr.n_reads < idx.ctx.n_reads         # labels of the real reads; the context holds chunks
    want = check(idx, lab)
    seam = np.flatnonzero((want['start'] == 60000) & (want['chrom'] == 0))[0]
    assert want['n_intervals'][seam] == 12 and want['n_reads'][seam] == 2     # 11 of the long read + read 2's
    with pytest.raises(_lib.FslrError, match=STATE):              # a table over the virtual reads is another n
        idx.ctx.cluster_table(np.arange(idx.ctx.n_reads, dtype=np.int32))
        idx.ctx.cluster_loci()
    got = idx.cluster_loci(lab)                                   # the wrapper's way in for host labels
    same_rows({k: getattr(got, k if k != 'chrom' else 'chrom_id') for k in ('off',) + lr.COLUMNS}, want)


# ------------------------------------------------------------------ 6. labels of a real query
def test_synth_query_resident_and_host_labels():
    from fslr_amd import synth
    from fslr_amd.prep import fold_overlap_threshold, pass_table
    csr = synth.generate(20_000, 16, 11).interval_data().csr()
    c = _lib.Context(0, profiling=True)
    try:
        c.load_csr(csr, fold_overlap_threshold(csr.iv_aln, 0.8))
        c.reserve_edges(max(1 << 16, 12 * csr.n_reads))
        c.build_index()
        c.run_query(0.96, 0.75, pass_table(CUTOFFS), 10)
        c.apply_edge_cap(10)
        c.components()
        labels = c.labels()
        c.cluster_table()
        resident = [device_rows(c), device_rows(c)]
        assert c.cluster_loci_timings()['loci'] > 0
        host = device_rows(c, labels)
        want = lr.loci_of_csr(csr, labels)
        assert len(want['start']) > 1000
        for got in resident + [host]:
            same_rows(got, want)
        assert [resident[0][k].tobytes() for k in want] == [resident[1][k].tobytes() for k in want]
    finally:
        c.close()


# ------------------------------------------------------------------ 7. golden fixtures
def fixture_membership(name):
    """The host pipeline's data and the reference's clusters: cid per read rank from its mappings.cluster.bed
    (clusters of two or more reads)."""
    from host_pipeline import host_prepare
    data, _, kw = host_prepare(name)
    csr = data.csr()
    names = np.asarray(data.qnames, dtype=object)[np.asarray(csr.read_qcode)]
    exp = pd.read_csv(io.StringIO(fx.expected_text(name, 'cluster')), sep='\t')
    exp = exp[exp['n_reads'] >= 2].drop_duplicates('qname')
    of = dict(zip(exp['qname'].tolist(), exp['cluster'].astype(np.int64).tolist()))
    cid = np.asarray([of.get(q, -1) for q in names.tolist()], np.int64)
    nc = int(cid.max()) + 1
    assert sorted(set(cid[cid >= 0].tolist())) == list(range(nc))
    return data, csr, cid, nc, kw


def query(idx, data, kw):
    return cluster.query_graph(idx, data, kw['overlap'], [float(x) for x in kw['jaccard_cutoffs'].split(',')], 10,
                               kw['qlen_diff'], kw['n_alignment_diff'])


@pytest.mark.parametrize('name', ['cfg1_1k_x3', 'ties_600', 'longreads_400'])
def test_golden_fixtures(name):
    data, csr, cid, nc, kw = fixture_membership(name)
    want = lr.loci(csr.read_off, csr.iv_chrom, csr.iv_start, csr.iv_end, cid, nc)
    idx = cluster.build_interval_trees(data)
    try:
        assert (idx.long is not None) == (name == 'longreads_400')
        g = query(idx, data, kw)
        got = idx.cluster_loci(g)
        assert isinstance(got, cluster.ClusterLoci) and len(got) == len(want['start']) > 0
        same_rows({k: getattr(got, k if k != 'chrom' else 'chrom_id') for k in ('off',) + lr.COLUMNS}, want)
        np.testing.assert_array_equal(idx._dense_chroms(got.chrom), got.chrom_id)     # the caller's values
        np.testing.assert_array_equal(got.cluster_of_row(), np.repeat(np.arange(nc), np.diff(want['off'])))
        assert list(got.to_frame().columns) == ['cluster', 'chrom', 'start', 'end', 'n_intervals', 'n_reads']
        if idx.long is None:                                       # the query's labels are resident
            idx.ctx.cluster_table()
            same_rows(device_rows(idx.ctx), want)
    finally:
        idx.ctx.close()


# ------------------------------------------------------------------ 8. protocol
def get_rows(c, n_clusters, capacity, fill=-7):
    off = np.full(n_clusters + 1, fill, np.int64)
    cols = [np.full(max(capacity, 1), fill, np.int32) for _ in range(5)]
    rc = c._L.fslr_get_cluster_loci(c._h, _lib._ptr(off), *(_lib._ptr(x) for x in cols), capacity)
    return rc, off, cols


def test_state_errors_and_the_previous_result():
    c = _lib.Context(0)
    try:
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*no reads'):
            c.cluster_loci()
        assert get_rows(c, 0, 0)[0] == _lib.FSLR_ERR_STATE
        idx, rng = random_index(c, 21, 400, 3, 3000)
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*no cluster table'):
            c.cluster_loci()
        n = idx.csr.n_reads
        lab = random_labels(rng, n)
        want = check(idx, lab)
        nc, nr = want['off'].size - 1, len(want['start'])
        with pytest.raises(_lib.FslrError, match=STATE):
            c.cluster_loci_timings()                              # not a profiling context
        # capacity
        rc, off, cols = get_rows(c, nc, nr - 1)
        assert rc == _lib.FSLR_ERR_INVALID and (off == -7).all() and all((x == -7).all() for x in cols)
        assert 'capacity' in c._L.fslr_last_error(c._h).decode()
        # NULL outputs are skipped
        start = np.empty(nr, np.int32)
        assert c._L.fslr_get_cluster_loci(c._h, None, None, _lib._ptr(start), None, None, None, nr) == _lib.FSLR_OK
        np.testing.assert_array_equal(start, want['start'])
        # reads again without an index: refused, and the rows made before still answer
        c.load_csr(idx.csr, np.zeros(idx.csr.n_intervals, np.int32))
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_build_index'):
            c.cluster_loci()
        rc, off, cols = get_rows(c, nc, nr)
        assert rc == _lib.FSLR_OK
        same_rows(dict(zip(('off',) + lr.COLUMNS, [off] + cols)), want)
        c.build_index()
        same_rows(device_rows(c), want)                           # the table outlived the upload: same n
        # a table of another n
        c.cluster_table(np.zeros(n + 3, np.int32))
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*{n + 3} reads.*{n}'):
            c.cluster_loci()
        # fslr_cluster_table dropped the rows
        assert get_rows(c, nc, nr)[0] == _lib.FSLR_ERR_STATE
        same_rows(device_rows(c, lab), want)
    finally:
        c.close()


def test_append_and_remove_leave_a_stale_table():
    data, csr, cid, nc, kw = fixture_membership('cfg1_1k_x3')
    codes = np.unique(data.qcode)
    late = np.isin(data.qcode, codes[codes.size * 2 // 3:])
    idx = cluster.build_interval_trees(data.select(~late))
    fresh = None
    try:
        c = idx.ctx
        first = idx.cluster_loci(query(idx, idx.data, kw))
        assert len(first) > 0
        idx.append(data.select(late))
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_table again'):
            c.cluster_loci()
        rc, off, cols = get_rows(c, first.off.size - 1, len(first))           # the rows made before still answer
        assert rc == _lib.FSLR_OK
        np.testing.assert_array_equal(cols[1], first.start)
        # a new query and table: the loci of a fresh upload of the same reads
        after = idx.cluster_loci(query(idx, idx.data, kw))
        fresh = cluster.build_interval_trees(idx.data)
        want = fresh.cluster_loci(query(fresh, fresh.data, kw))
        for k in ('off', 'chrom', 'chrom_id') + lr.COLUMNS[1:]:
            np.testing.assert_array_equal(getattr(after, k), getattr(want, k), err_msg=k)
        same_rows({k: getattr(after, k if k != 'chrom' else 'chrom_id') for k in ('off',) + lr.COLUMNS},
                  lr.loci_of_csr(idx.csr, c.labels()))
        keep = np.ones(idx.csr.n_reads, bool)
        keep[::7] = False
        idx.remove(keep=keep)
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_table again'):
            c.cluster_loci()
        lab = np.zeros(idx.csr.n_reads, np.int32)
        same_rows(device_rows(c, lab), lr.loci_of_csr(idx.csr, lab))
    finally:
        idx.ctx.close()
        if fresh is not None:
            fresh.ctx.close()


def test_multi_gpu_index_refuses():
    mg = cluster.MultiGpuIndex(sr.make_data([1, 1], [0, 5], [9, 9]), 2)
    with pytest.raises(NotImplementedError, match='n_gpus=1'):
        mg.cluster_loci()


# ------------------------------------------------------------------ 9. the command line
def run_cli(name, tmp, *flags):
    from click.testing import CliRunner
    from fslr_amd.main import pipeline
    with open(os.path.join(tmp, 'fx.mappings.bed'), 'w') as fh:
        fh.write(fx.input_bed_text(name))
    shutil.copy(fx.input_bam(name), os.path.join(tmp, 'fx.bwa_dodi.bam'))
    args = ['--name', 'fx', '--out', str(tmp), '--ref', 'unused.fa', '--primers', '21q1', '--skip-alignment'] + \
        fx.meta(name)['args'] + list(flags)
    return CliRunner().invoke(pipeline, args, catch_exceptions=True)


@pytest.mark.parametrize('io_flag', ['--native-io', '--pandas-io'])
def test_cli_cluster_loci(tmp_path, io_flag):
    name = 'cfg1_1k_x3'
    data, csr, cid, nc, kw = fixture_membership(name)
    cmap = fastcli.chrom_map(list(pd.unique(fx.input_bed(name)['chrom'])))
    name_of = {v: k for k, v in cmap.items()}
    dense_names = [name_of[v] for v in np.unique(data.chrom).tolist()]
    want = lr.bed_text(lr.loci(csr.read_off, csr.iv_chrom, csr.iv_start, csr.iv_end, cid, nc), dense_names)
    tmp = str(tmp_path)
    res = run_cli(name, tmp, io_flag, '--cluster-loci')
    assert res.exit_code == 0, (res.output, res.exception)
    assert open(os.path.join(tmp, 'fx.mappings.cluster_loci.bed')).read() == want
    for which in ('cluster', 'representative'):
        assert open(os.path.join(tmp, f'fx.mappings.{which}.bed')).read() == fx.expected_text(name, which), which
    os.remove(os.path.join(tmp, 'fx.mappings.cluster_loci.bed'))
    res = run_cli(name, tmp, io_flag)
    assert res.exit_code == 0, (res.output, res.exception)
    assert sorted(os.listdir(tmp)) == ['fx.bwa_dodi.bam', 'fx.mappings.bed', 'fx.mappings.cluster.bed',
                                       'fx.mappings.representative.bed']
    for which in ('cluster', 'representative'):
        assert open(os.path.join(tmp, f'fx.mappings.{which}.bed')).read() == fx.expected_text(name, which), which


def test_cli_long_reads_upload_their_labels(tmp_path):
    name = 'longreads_400'
    data, csr, cid, nc, kw = fixture_membership(name)
    cmap = fastcli.chrom_map(list(pd.unique(fx.input_bed(name)['chrom'])))
    name_of = {v: k for k, v in cmap.items()}
    dense_names = [name_of[v] for v in np.unique(data.chrom).tolist()]
    want = lr.bed_text(lr.loci(csr.read_off, csr.iv_chrom, csr.iv_start, csr.iv_end, cid, nc), dense_names)
    res = run_cli(name, str(tmp_path), '--cluster-loci')
    assert res.exit_code == 0, (res.output, res.exception)
    assert open(os.path.join(str(tmp_path), 'fx.mappings.cluster_loci.bed')).read() == want


def test_cli_refuses_several_gpus(tmp_path):
    res = run_cli('cfg1_1k_x3', str(tmp_path), '--cluster-loci', '--gpus=2')
    assert res.exit_code == 2 and '--gpus 1' in res.output
    assert sorted(os.listdir(str(tmp_path))) == ['fx.bwa_dodi.bam', 'fx.mappings.bed']
