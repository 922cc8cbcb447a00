"""calc_coverage / filter_high_coverage (cluster.py:52-77) without a device: the host path against the
reference's own results (tests/golden/coverage/small.npz, made by make_coverage_golden.py), the identity
the device path rests on, and the host side of the device path (row filter, dense ids, numpy's index
rules, the reference's exceptions) over a stand-in context that answers with numpy."""
import os

import numpy as np
import pandas as pd
import pytest

from fslr_amd import cluster
from fslr_amd.prep import IntervalData, IntervalItem

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'coverage', 'small.npz')


@pytest.fixture(scope='module')
def g():
    return dict(np.load(GOLDEN))


def lengths(g):
    return dict(zip(g['len_chrom'].tolist(), g['len_value'].tolist()))


def bed(g, prefix='bed'):
    return pd.DataFrame({'chrom': g[f'{prefix}_chrom'], 'rstart': g[f'{prefix}_rstart'], 'rend': g[f'{prefix}_rend']})


def data_items(g):
    cols = [g[f'data_{c}'].tolist() for c in ('chrom', 'start', 'end', 'aln_size')]
    rest = [g[f'data_{c}'].tolist() for c in ('n_alignments', 'qlen2', 'middle', 'index')]
    return [IntervalItem(*(c[i] for c in cols), f'q{rest[3][i]}', *(c[i] for c in rest)) for i in range(len(cols[0]))]


def upper_bounds_depth(chrom, rstart, rend, qchrom, qpos):
    """#{rstart keys <= q} - #{rend keys <= q} over chrom << 32 | pos keys of all chromosomes at once."""
    ks = np.sort(np.asarray(chrom, np.int64) << 32 | np.asarray(rstart, np.int64))
    ke = np.sort(np.asarray(chrom, np.int64) << 32 | np.asarray(rend, np.int64))
    q = np.asarray(qchrom, np.int64) << 32 | np.asarray(qpos, np.int64)
    return (np.searchsorted(ks, q, side='right') - np.searchsorted(ke, q, side='right')).astype(np.int32)


class NumpyContext:
    """Context's coverage calls answered on the host (the device's contract: dense ids, positions >= 0)."""
    coverage_gen = 0

    def coverage_build(self, chrom, rstart, rend, n_chroms):
        rows = [np.asarray(x, np.int64) for x in (chrom, rstart, rend)]
        assert all((x >= 0).all() for x in rows) and (rows[0] < n_chroms).all()
        self.rows, self.n_chroms = rows, n_chroms
        self.coverage_gen += 1

    def coverage_at(self, chrom, pos):
        chrom, pos = np.asarray(chrom), np.asarray(pos)
        assert chrom.dtype == pos.dtype == np.int32 and (chrom >= 0).all() and (chrom < self.n_chroms).all()
        assert (pos >= 0).all()
        return upper_bounds_depth(*self.rows, chrom, pos)

    def close(self):
        raise AssertionError("a caller's context is not closed")


def test_golden_file_is_small_and_covers_the_cases(g):
    assert os.path.getsize(GOLDEN) < 100_000
    L = lengths(g)
    c, a, b = g['bed_chrom'], g['bed_rstart'], g['bed_rend']
    assert 1900 <= c.size <= 2100 and sorted(L) == [1, 2, 5, 7] and sorted(set(c.tolist())) == [1, 2, 5, 9]
    assert (a == b).sum() >= 20 and (a > b).sum() >= 100
    for k in (1, 2, 5):
        m = c == k
        assert (a[m] == 0).any() and (a[m] == L[k]).any() and (b[m] == 0).any() and (b[m] == L[k]).any()
        assert g[f'cov_{k}'].shape == (L[k] + 1,)
    assert min(g[f'cov_{k}'].min() for k in (1, 2, 5)) < -5


def test_host_calc_coverage_is_the_reference(g):
    cov = cluster.calc_coverage(bed(g), lengths(g))
    assert sorted(cov) == [1, 2, 5]
    for k, v in cov.items():
        assert v.dtype == np.float64
        np.testing.assert_array_equal(v, g[f'cov_{k}'].astype(np.float64))
    for k, v in cluster.calc_coverage(bed(g, 'wrap'), lengths(g)).items():
        np.testing.assert_array_equal(v, g[f'wrap_cov_{k}'].astype(np.float64))


def test_host_filter_is_the_reference(g):
    items = data_items(g)
    data = IntervalData.from_items(items)
    for k, t in enumerate(g['thresholds'].tolist()):
        kept = cluster.filter_high_coverage(items, bed(g), lengths(g), t)
        assert [items.index(x) for x in kept] == g[f'kept_{k}'].tolist()
        sel = cluster.filter_high_coverage(data, bed(g), lengths(g), t)
        np.testing.assert_array_equal(sel.index, g['data_index'][g[f'kept_{k}']])


def test_two_upper_bounds_give_the_dense_arrays(g):
    c, a, b = g['bed_chrom'], g['bed_rstart'], g['bed_rend']
    for k in (1, 2, 5):                      # chromosome 9's rows (no length) and the lower chromosomes' cancel
        pos = np.arange(g[f'cov_{k}'].size)
        np.testing.assert_array_equal(upper_bounds_depth(c, a, b, np.full(pos.size, k), pos), g[f'cov_{k}'])


def test_device_path_host_side(g):
    """Row filter, dense ids, wrap and the dict / array behaviour, the arithmetic done by numpy."""
    L = lengths(g)
    ctx = NumpyContext()
    cov = cluster.calc_coverage(bed(g), L, ctx=ctx)
    assert isinstance(cov, cluster.DeviceCoverage) and ctx.n_chroms == 3 and ctx.rows[0].size == (g['bed_chrom'] != 9).sum()
    assert list(cov.keys()) == [1, 2, 5] and len(cov) == 3 and 5 in cov and 7 not in cov and 9 not in cov
    for k in (1, 2, 5):
        want = g[f'cov_{k}'].astype(np.float64)
        assert len(cov[k]) == L[k] + 1
        got = cov[k][:]
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(cov[k][-5:], want[-5:])
        np.testing.assert_array_equal(cov[k][10:700:7], want[10:700:7])
        idx = np.array([0, -1, L[k], -L[k] - 1, 3])
        np.testing.assert_array_equal(cov[k][idx], want[idx])
        v = cov[k][-2]
        assert type(v) is float and v == want[-2] and cov[k][np.int64(7)] == want[7]
        for p in (L[k] + 1, -L[k] - 2):
            with pytest.raises(IndexError):
                cov[k][p]
            with pytest.raises(IndexError):
                cov[k][np.array([0, p])]
    for k in (7, 9, 'chr1'):
        with pytest.raises(KeyError):
            cov[k]
    d = cov.depth_at(g['data_chrom'], g['data_middle'])
    assert d.dtype == np.int32
    np.testing.assert_array_equal(d, [g[f'cov_{c}'][m] for c, m in zip(g['data_chrom'].tolist(), g['data_middle'].tolist())])
    assert cov.depth_at([], []).shape == (0,)
    # negative bed positions wrap before the upload
    w = cluster.device_coverage(bed(g, 'wrap'), L, ctx=ctx)
    for k in (2, 5):
        np.testing.assert_array_equal(w[k][:], g[f'wrap_cov_{k}'].astype(np.float64))
    with pytest.raises(RuntimeError, match='rebuilt'):
        cov[1][0]
    # string labels (before rename_chromosomes)
    names = {1: 'chr1', 2: 'chr2', 5: 'chrX', 7: 'chr7', 9: 'chrUn'}
    b = bed(g)
    b['chrom'] = b['chrom'].map(names)
    s = cluster.calc_coverage(b, {names[k]: v for k, v in L.items()}, ctx=ctx)
    assert list(s.keys()) == ['chr1', 'chr2', 'chrX']
    np.testing.assert_array_equal(s['chrX'][:], g['cov_5'].astype(np.float64))
    np.testing.assert_array_equal(s.depth_at(['chrX', 'chr1'], [3, 1500]), [g['cov_5'][3], g['cov_1'][1500]])


def test_device_filter_host_side(g):
    items = data_items(g)
    data = IntervalData.from_items(items)
    ctx = NumpyContext()
    for k, t in enumerate(g['thresholds'].tolist()):
        kept = cluster.filter_high_coverage(items, bed(g), lengths(g), t, ctx=ctx)
        assert kept == [items[i] for i in g[f'kept_{k}'].tolist()]
        sel = cluster.filter_high_coverage(data, bed(g), lengths(g), t, ctx=ctx)
        np.testing.assert_array_equal(sel.index, g['data_index'][g[f'kept_{k}']])
    assert cluster.filter_high_coverage([], bed(g), lengths(g), 5, ctx=ctx) == []


@pytest.mark.parametrize('device', [False, True])
def test_the_reference_s_exceptions(g, device):
    """Every input the golden generator saw the reference raise on raises the same class here: on the host
    path and, before anything is uploaded or asked of the device, on the device path."""
    assert int(g['n_err']) == 7
    seen = set()
    for k in range(int(g['n_err'])):
        exc = {'IndexError': IndexError, 'KeyError': KeyError}[str(g[f'err{k}_type'])]
        seen.add(exc)
        items = [IntervalItem(c, 0, 1, 1, 'q', 3, 100, m, i)
                 for i, (c, m) in enumerate(zip(g[f'err{k}_data_chrom'].tolist(), g[f'err{k}_data_middle'].tolist()))]
        kw = {'ctx': NumpyContext()} if device else {}
        rows, L = bed(g, f'err{k}_bed'), lengths(g)
        for data in (items, IntervalData.from_items(items)):
            with pytest.raises(exc):
                cluster.filter_high_coverage(data, rows, L, 10, **kw)
    assert seen == {IndexError, KeyError}
