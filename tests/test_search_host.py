"""The batched search's interface without a device: the brute-force expectation the GPU tests use
agrees with the superintervals stand-in (search_values' predicate and order), the library exports the
new calls and they reject a null context, and the index classes carry the new methods."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import refharness
import search_ref as sr
from fslr_amd import _lib, cluster

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_brute_force_agrees_with_the_stand_in():
    """200 random queries over 3 chromosomes and 2000 intervals with heavy start ties: the same data
    positions in the same order as refharness._IntervalMap (one map per chromosome, filled in `data`
    order, as build_interval_trees fills it, cluster.py:124-130)."""
    rng = np.random.default_rng(17)
    n = 2000
    chrom = rng.integers(1, 4, n)
    start = rng.integers(0, 120, n) * 50                       # ~17 intervals per start value
    end = start + rng.integers(0, 6, n) * 100 + rng.integers(0, 2, n)
    data = sr.make_data(chrom, start, end, shuffle_seed=3)
    trees = {}
    for p, (c, s, e) in enumerate(zip(data.chrom.tolist(), data.start.tolist(), data.end.tolist())):
        trees.setdefault(c, refharness._IntervalMap()).add(s, e, p)
    qc = rng.integers(1, 5, 200)                               # 4: a chromosome the data lacks
    qs = rng.integers(-100, 6500, 200)
    qe = qs + rng.integers(-50, 900, 200)                      # some with qs > qe
    off, pos = sr.brute_force(data.chrom, data.start, data.end, qc, qs, qe)
    assert off[-1] > 1000
    ties = 0
    for k, (c, s, e) in enumerate(zip(qc.tolist(), qs.tolist(), qe.tolist())):
        want = trees[c].search_values(s, e) if c in trees else []
        got = pos[off[k]:off[k + 1]].tolist()
        assert got == want, (k, c, s, e)
        ties += len(got) - len(set(data.start[got].tolist())) if got else 0
    assert ties > 500                                          # the order inside runs of equal start was tested


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(['make', '-s', '-C', os.path.join(REPO, 'fslr_amd', 'csrc')], check=True)
    return _lib.load()


def test_search_symbols_reject_a_null_context(lib):
    for name in ('fslr_search', 'fslr_search_hits', 'fslr_search_timings'):
        assert name in _lib.EXPORTED and hasattr(lib, name), name
    total = ctypes.c_int64(-1)
    assert lib.fslr_search(None, 0, None, None, None, None, ctypes.byref(total)) == _lib.FSLR_ERR_INVALID
    assert lib.fslr_search_hits(None, None, 0) == _lib.FSLR_ERR_INVALID
    assert lib.fslr_search_timings(None, None) == _lib.FSLR_ERR_INVALID
    assert total.value == -1


def test_index_classes_have_the_search_interface():
    for name in ('search_batch', 'count_batch', '__getitem__', '__contains__', 'keys', 'items'):
        assert callable(getattr(cluster.DeviceIntervalIndex, name)), name
        assert callable(getattr(cluster.RowsIndex, name)), name
    for name in ('search', 'search_counts'):
        assert callable(getattr(_lib.Context, name)), name
    for name in ('search_values', 'search_idxs', 'count'):
        assert callable(getattr(cluster.ChromosomeView, name)), name


def test_multi_gpu_index_declines_search():
    data = sr.make_data([1, 1], [10, 20], [30, 40])
    mg = cluster.build_interval_trees(data, n_gpus=2)
    assert isinstance(mg, cluster.MultiGpuIndex)
    for call in (lambda: mg.search_batch([1], [0], [5]), lambda: mg.count_batch([1], [0], [5]), lambda: mg[1]):
        with pytest.raises(NotImplementedError, match='rank processes'):
            call()


def test_coordinates_are_clipped_and_chromosomes_mapped_once():
    """The host side of search_batch: the clip to [-1, 2**30] and the caller's chromosome values to
    dense ids (-1 for one the index lacks), without a device."""
    idx = object.__new__(cluster.DeviceIntervalIndex)
    idx.source = idx.data = sr.make_data([5, 2, 9, 2], [10, 20, 30, 40], [15, 25, 35, 45])
    idx.csr = idx.data.csr()
    np.testing.assert_array_equal(idx._dense_chroms(np.array([2, 5, 9, 7, -3])), [0, 1, 2, -1, -1])
    np.testing.assert_array_equal(idx._dense_chroms([9]), [2])
    assert idx._chrom_table() is idx._chrom_table()
    assert 5 in idx and 7 not in idx and sorted(idx.keys()) == [2, 5, 9]
    c = idx._coords([-5, -1, 0, (1 << 30) - 1, 1 << 30, 1 << 40, -(1 << 40)])
    assert c.dtype == np.int32
    np.testing.assert_array_equal(c, [-1, -1, 0, (1 << 30) - 1, 1 << 30, 1 << 30, -1])
    items = list(idx.data)
    idx2 = object.__new__(cluster.DeviceIntervalIndex)
    idx2.source = [it._replace(chrom=f'chr{it.chrom}') for it in items]       # names, as an unrenamed list has
    from fslr_amd.prep import IntervalData
    idx2.data = IntervalData.from_items(idx2.source)
    idx2.csr = idx2.data.csr()
    got = idx2._dense_chroms(['chr2', 'chrX', 'chr9'])
    assert got[1] == -1 and got[0] != got[2] and min(got[0], got[2]) >= 0
    assert idx2.csr.iv_chrom[np.flatnonzero(idx2.csr.data_pos == 1)[0]] == got[0]    # data position 1 is on chr2
