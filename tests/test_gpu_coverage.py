"""Read depth on the device (fslr_coverage_build / fslr_coverage_at, cluster.device_coverage): the
reference's calc_coverage / filter_high_coverage (cluster.py:52-77) against its own dense arrays
(tests/golden/coverage/small.npz) and against np.searchsorted, at the kernel's tile, run and chunk
boundaries."""
import ctypes
import os

import numpy as np
import pandas as pd
import pytest

from fslr_amd import _lib, cluster, synth
from fslr_amd.prep import IntervalData, IntervalItem, fold_overlap_threshold, pass_table

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'coverage', 'small.npz')
T = _lib.COVERAGE_TILE
CHUNK = _lib.COVERAGE_CHUNK
CUTOFFS = (1, 1, 0.66, 0.66, 0.66, 0.5)


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def g():
    return dict(np.load(GOLDEN))


def lengths(g):
    return dict(zip(g['len_chrom'].tolist(), g['len_value'].tolist()))


def bed(chrom, rstart, rend):
    return pd.DataFrame({'chrom': chrom, 'rstart': rstart, 'rend': rend})


def golden_bed(g):
    return bed(g['bed_chrom'], g['bed_rstart'], g['bed_rend'])


def host_depth(chrom, rstart, rend, qchrom, qpos):
    """The two upper bounds by np.searchsorted (test_coverage_host.py pins them to the reference)."""
    ks = np.sort(np.asarray(chrom, np.int64) << 32 | np.asarray(rstart, np.int64))
    ke = np.sort(np.asarray(chrom, np.int64) << 32 | np.asarray(rend, np.int64))
    q = np.asarray(qchrom, np.int64) << 32 | np.asarray(qpos, np.int64)
    return np.searchsorted(ks, q, side='right') - np.searchsorted(ke, q, side='right')


def vp(x):
    return x.ctypes.data_as(ctypes.c_void_p)


# ------------------------------------------------------------------ 1. every position of the golden input
def test_exhaustive_against_the_reference(ctx, g):
    L = lengths(g)
    cov = cluster.calc_coverage(golden_bed(g), L, ctx=ctx)
    assert isinstance(cov, cluster.DeviceCoverage) and list(cov.keys()) == [1, 2, 5]
    qc = np.concatenate([np.full(L[k] + 1, k) for k in (1, 2, 5)])
    qp = np.concatenate([np.arange(L[k] + 1) for k in (1, 2, 5)])
    want = np.concatenate([g[f'cov_{k}'] for k in (1, 2, 5)]).astype(np.int64)
    order = np.random.default_rng(5).permutation(qc.size)
    got = cov.depth_at(qc[order], qp[order])
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got.astype(np.int64), want[order])
    assert want.min() < -5 and want.max() > 60
    for k in (1, 2, 5):
        dense = g[f'cov_{k}'].astype(np.float64)
        np.testing.assert_array_equal(cov[k][:], dense)
        np.testing.assert_array_equal(cov[k][17:701:3], dense[17:701:3])
        idx = np.array([0, L[k], -1, -L[k] - 1, 5, 5, 300])
        np.testing.assert_array_equal(cov[k][idx], dense[idx])
        for p in (0, L[k], -1, 299):
            v = cov[k][p]
            assert type(v) is float and v == dense[p]
        assert len(cov[k]) == L[k] + 1
        with pytest.raises(IndexError):
            cov[k][L[k] + 1]
    for k in (7, 9):
        with pytest.raises(KeyError):
            cov[k]


def test_filter_on_the_golden_input(ctx, g):
    """filter_high_coverage(..., ctx=ctx) returns the reference's list, as the host path does."""
    cols = [g[f'data_{c}'].tolist() for c in ('chrom', 'start', 'end', 'aln_size', 'n_alignments', 'qlen2', 'middle',
                                              'index')]
    items = [IntervalItem(*(c[i] for c in cols[:4]), f'q{cols[7][i]}', *(c[i] for c in cols[4:]))
             for i in range(len(cols[0]))]
    data = IntervalData.from_items(items)
    for k, t in enumerate(g['thresholds'].tolist()):
        want = [items[i] for i in g[f'kept_{k}'].tolist()]
        assert cluster.filter_high_coverage(items, golden_bed(g), lengths(g), t, ctx=ctx) == want
        assert cluster.filter_high_coverage(items, golden_bed(g), lengths(g), t) == want
        sel = cluster.filter_high_coverage(data, golden_bed(g), lengths(g), t, ctx=ctx)
        np.testing.assert_array_equal(sel.index, g['data_index'][g[f'kept_{k}']])
        assert 0 < len(want) < len(items)


# ------------------------------------------------------------------ 2. tiles and runs of equal keys
@pytest.mark.parametrize('n', [T - 1, T, T + 1, 2 * T + 1])
def test_row_counts_around_the_tile(ctx, n):
    rng = np.random.default_rng(n)
    chrom = rng.integers(0, 3, n)
    rs, re_ = rng.integers(5, 400, n), rng.integers(5, 400, n)
    ctx.coverage_build(chrom, rs, re_, 3)
    qc = np.repeat(np.arange(3), 410)
    qp = np.tile(np.arange(410), 3)                     # below the smallest key, every key, above the largest
    np.testing.assert_array_equal(ctx.coverage_at(qc, qp), host_depth(chrom, rs, re_, qc, qp))


@pytest.mark.parametrize('column', ['rstart', 'rend'])
def test_run_of_equal_keys_across_tiles(ctx, column):
    """2T + 37 rows share one position; the run starts mid-tile and crosses two tile boundaries."""
    run, before, after = 2 * T + 37, T // 2 + 3, T + 11
    rng = np.random.default_rng(7)
    pos = np.concatenate([rng.integers(10, 5000, before), np.full(run, 5000), rng.integers(5001, 9000, after)])
    other = rng.integers(10, 9000, pos.size)
    chrom = np.ones(pos.size, np.int64)
    rs, re_ = (pos, other) if column == 'rstart' else (other, pos)
    first = int(np.searchsorted(np.sort(pos), 5000))
    assert first % T != 0 and first // T + 2 <= (first + run - 1) // T       # mid-tile, two boundaries inside
    perm = rng.permutation(pos.size)
    ctx.coverage_build(chrom[perm], rs[perm], re_[perm], 2)
    qp = np.array([0, 9, 4999, 5000, 5001, 8999, 9000, 2 ** 31 - 1, int(pos.min()) - 1, int(pos.max()) + 1])
    qc = np.ones(qp.size, np.int64)
    got = ctx.coverage_at(qc, qp)
    np.testing.assert_array_equal(got, host_depth(chrom, rs, re_, qc, qp))
    # chromosome 0 has no rows: below every key; the positions above every key of chromosome 1 give 0
    assert ctx.coverage_at([0, 0], [0, 2 ** 31 - 1]).tolist() == [0, 0] and got[7] == 0


# ------------------------------------------------------------------ 3. half-open ends
def test_half_open_ends(ctx):
    #          a row      an empty row   a reversed row
    rows = [(0, 100, 200), (0, 150, 150), (1, 60, 40)]
    ctx.coverage_build(*(np.array(c) for c in zip(*rows)), 2)
    q = [(0, 99, 0), (0, 100, 1), (0, 149, 1), (0, 150, 1), (0, 151, 1), (0, 199, 1), (0, 200, 0), (0, 201, 0),
         (1, 39, 0), (1, 40, -1), (1, 41, -1), (1, 59, -1), (1, 60, 0), (1, 61, 0)]
    got = ctx.coverage_at([x[0] for x in q], [x[1] for x in q])
    assert got.tolist() == [x[2] for x in q]


# ------------------------------------------------------------------ 4. the filter's boundary
@pytest.mark.parametrize('n_rows,kept', [(10_000, True), (10_001, False)])
def test_threshold_boundary(ctx, n_rows, kept):
    """The reference drops only depth > threshold (cluster.py:74): 10,000 rows over a locus stay."""
    L = {1: 50_000, 2: 50_000}
    b = bed(np.concatenate([np.ones(n_rows, np.int64), [2]]), np.concatenate([np.full(n_rows, 20_000), [10]]),
            np.concatenate([np.full(n_rows, 21_000), [90]]))
    items = [IntervalItem(1, 20_400, 20_600, 200, 'in', 4, 900, 20_500, 0),
             IntervalItem(1, 30_400, 30_600, 200, 'out', 4, 900, 30_500, 1),
             IntervalItem(1, 20_900, 21_100, 200, 'end', 4, 900, 21_000, 2),
             IntervalItem(2, 10, 90, 80, 'other', 4, 900, 50, 3)]
    want = [x for x in items if kept or x.qname != 'in']
    assert cluster.filter_high_coverage(items, b, L, 10_000, ctx=ctx) == want
    assert cluster.filter_high_coverage(items, b, L, 10_000) == want
    data = IntervalData.from_items(items)
    dev = cluster.filter_high_coverage(data, b, L, 10_000, ctx=ctx)
    host = cluster.filter_high_coverage(data, b, L, 10_000)
    np.testing.assert_array_equal(dev.index, host.index)
    np.testing.assert_array_equal(dev.index, [x.index for x in want])
    assert ctx.coverage_at([0], [20_500]).tolist() == [n_rows]


# ------------------------------------------------------------------ 5. batch and row counts
def test_batch_sizes(ctx):
    rng = np.random.default_rng(21)
    n = 3 * T + 19
    chrom, rs, re_ = rng.integers(0, 4, n), rng.integers(0, 2000, n), rng.integers(0, 2000, n)
    ctx.coverage_build(chrom, rs, re_, 4)
    for nq in (0, 1, 63, 64, 65, CHUNK + 1):            # the last crosses a chunk boundary
        qc, qp = rng.integers(0, 4, nq), rng.integers(0, 2100, nq)
        got = ctx.coverage_at(qc, qp)
        assert got.shape == (nq,) and got.dtype == np.int32
        np.testing.assert_array_equal(got, host_depth(chrom, rs, re_, qc, qp))


def test_no_rows_and_one_row(ctx):
    z = np.zeros(0, np.int32)
    ctx.coverage_build(z, z, z, 3)
    assert ctx.coverage_at([0, 1, 2, 2], [0, 5, 2 ** 31 - 1, 7]).tolist() == [0, 0, 0, 0]
    ctx.coverage_build(z, z, z, 0)
    assert ctx.coverage_at(z, z).shape == (0,)
    ctx.coverage_build([1], [10], [12], 2)
    assert ctx.coverage_at([0, 1, 1, 1, 1, 1], [11, 9, 10, 11, 12, 13]).tolist() == [0, 0, 1, 1, 0, 0]
    cov = cluster.device_coverage(bed(z, z, z), {1: 100}, ctx=ctx)
    assert len(cov) == 0 and 1 not in cov


# ------------------------------------------------------------------ 6. errors
def test_query_before_build_is_a_state_error():
    c = _lib.Context(0)
    try:
        with pytest.raises(_lib.FslrError, match=f'fslr error {_lib.FSLR_ERR_STATE}.*fslr_coverage_build'):
            c.coverage_at([0], [0])
        with pytest.raises(_lib.FslrError, match=f'fslr error {_lib.FSLR_ERR_STATE}'):
            c.coverage_timings()
    finally:
        c.close()


def test_bad_arguments_write_nothing_and_keep_the_set(ctx):
    ctx.coverage_build([0, 1, 1], [5, 10, 20], [9, 30, 25], 2)
    q = (np.array([0, 1, 1], np.int32), np.array([6, 22, 30], np.int32))
    want = ctx.coverage_at(*q)
    assert want.tolist() == [1, 2, 0]
    for qc, qp, where in (([0, 2, 1], [6, 22, 30], 'query 1'), ([0, 1, -1], [6, 22, 30], 'query 2'),
                          ([0, 1, 1], [-6, 22, 30], 'query 0')):
        qc, qp = np.array(qc, np.int32), np.array(qp, np.int32)
        depth = np.full(3, -77, np.int32)
        rc = ctx._L.fslr_coverage_at(ctx._h, 3, vp(qc), vp(qp), vp(depth))
        assert rc == _lib.FSLR_ERR_INVALID and where in ctx._L.fslr_last_error(ctx._h).decode()
        assert (depth == -77).all()
    # a failed rebuild leaves the previous coverage answering
    gen = ctx.coverage_gen
    for chrom, rs, re_, where in (([0, 1, 2], [1, 2, 3], [4, 5, 6], 'row 2'), ([0, -1, 5], [1, 2, 3], [4, 5, 6], 'row 1'),
                                  ([0, 1, 1], [1, 2, -3], [4, 5, 6], 'row 2'), ([0, 1, 1], [1, 2, 3], [-4, 5, -6], 'row 0')):
        with pytest.raises(_lib.FslrError, match=f'fslr error {_lib.FSLR_ERR_INVALID}.*{where} '):
            ctx.coverage_build(chrom, rs, re_, 2)
        assert ctx.coverage_gen == gen
        np.testing.assert_array_equal(ctx.coverage_at(*q), want)


# ------------------------------------------------------------------ 7. independence of the other state
def test_leaves_the_query_and_search_state_alone():
    s = synth.generate(3000, 16, 11)
    data = s.interval_data()
    csr = data.csr()
    pt = pass_table(CUTOFFS)
    c = _lib.Context(0)
    try:
        c.load_csr(csr, fold_overlap_threshold(csr.iv_aln, 0.8))
        c.reserve_edges(12 * csr.n_reads)
        c.build_index()

        def graph():
            st = c.run_query(1 - 0.04, 1 - 0.25, pt, engine='sweep')
            c.components()
            return st, (*c.edges(st['n_edges']), c.fwd_degree(), c.labels())
        st0, before = graph()
        assert st0['engine'] == 'sweep' and st0['n_edges'] > 100
        stats0 = c.stats()
        dense = np.asarray(csr.iv_chrom[:300], np.int32)
        qs, qe = np.asarray(csr.iv_start[:300], np.int32), np.asarray(csr.iv_end[:300], np.int32)
        _, want_hits = c.search(dense, qs, qe)
        total = c._search(dense, qs, qe, None)
        assert total == want_hits.size > 300
        # coverage of the bed rows the reads came from, queried at the prepared data's middles
        df = s.to_dataframe()
        names = {n: k + 1 for k, n in enumerate(synth.CHROMS)}
        df['chrom'] = df['chrom'].map(names)
        L = {names[k]: v for k, v in s.chrom_lengths.items()}
        cov = cluster.calc_coverage(df, L, ctx=c)
        depth = cov.depth_at(data.chrom, data.middle)
        np.testing.assert_array_equal(depth, host_depth(df['chrom'], df['rstart'], df['rend'], data.chrom, data.middle))
        assert depth.min() >= 1 and depth.max() >= 2
        hits = np.full(total, -7, np.int32)
        c._check(c._L.fslr_search_hits(c._h, vp(hits), total))
        np.testing.assert_array_equal(hits, want_hits)
        assert c.stats() == stats0
        for x, y in zip(before, (*c.edges(st0['n_edges']), c.fwd_degree(), c.labels())):
            np.testing.assert_array_equal(x, y)
        st1, after = graph()
        assert st1['n_edges'] == st0['n_edges']
        for x, y in zip(before[4:], after[4:]):
            np.testing.assert_array_equal(x, y)
        e0 = sorted(zip(*(x.tolist() for x in before[:4])))
        assert sorted(zip(*(x.tolist() for x in after[:4]))) == e0
        np.testing.assert_array_equal(cov.depth_at(data.chrom, data.middle), depth)
    finally:
        c.close()
    # a context that never had reads
    f = _lib.Context(0)
    try:
        f.coverage_build([0, 0], [3, 4], [8, 6], 1)
        assert f.coverage_at([0, 0, 0], [3, 5, 7]).tolist() == [1, 2, 1]
    finally:
        f.close()


# ------------------------------------------------------------------ 8. determinism, timings
def test_two_rounds_give_the_same_bytes():
    rng = np.random.default_rng(3)
    n = 50_000
    chrom, rs, re_ = rng.integers(0, 5, n), rng.integers(0, 30_000, n), rng.integers(0, 30_000, n)
    rs[:7000] = 12_345                                  # a pile
    qc, qp = rng.integers(0, 5, 200_000), rng.integers(0, 30_100, 200_000)
    out = []
    for _ in range(2):
        c = _lib.Context(0, profiling=True)
        try:
            c.coverage_build(chrom, rs, re_, 5)
            out.append(c.coverage_at(qc, qp).tobytes())
            t = c.coverage_timings()
            assert sorted(t) == ['build_sort', 'build_upload', 'query_download', 'query_upload_kernel']
            assert all(v > 0 for v in t.values())
        finally:
            c.close()
    assert out[0] == out[1]
    np.testing.assert_array_equal(np.frombuffer(out[0], np.int32), host_depth(chrom, rs, re_, qc, qp))
