"""Cluster junctions for reads of more than 64 intervals (fslr_cluster_junctions_any) against tests/junctions_ref.py,
which states the contract for lists of any length.  Hand-built inputs of a handful of reads; every comparison is
exact, dtypes included."""
import numpy as np
import pytest

import chain_any_cases as cc
import junctions_ref as jr
import loci_ref as lr
from fslr_amd import _lib, cluster
from test_gpu_junctions import get_rows, resident_equals, same_rows
from test_gpu_loci import fixture_membership, query

pytestmark = pytest.mark.gpu

STATE = f'fslr error {_lib.FSLR_ERR_STATE}'
INVALID = f'fslr error {_lib.FSLR_ERR_INVALID}'
NAMES = ('off',) + jr.COLUMNS
# the lengths around the chunk seams and the limit, short reads between them; the read of 70 is left alone
LENS = (64, 65, 128, 129, 1000, 4096, 3, 2, 1, 70, 17)
ALONE = 9


def rows_any(c, qkey, rev=None, labels=None, loci=True):
    if labels is not None:
        c.cluster_table(labels)
    if loci:
        c.cluster_loci()
    return dict(zip(NAMES, c.cluster_junctions_any(qkey, rev)))


def check(idx, labels, qkey, rev=None):
    want = jr.junctions_of_csr(idx.csr, labels, qkey, rev)
    same_rows(rows_any(idx.ctx, qkey, rev, labels), want)
    return want


@pytest.fixture(scope='module')
def mixed():
    """One cluster of all of LENS but the read of 70 intervals."""
    c = _lib.Context(0)
    idx = cc.index_of_lens(c, LENS, seed=5)
    yield idx, cc.one_cluster(idx.csr, alone=(ALONE,))
    c.close()


# ------------------------------------------------------------------ 1. lengths and key orders
@pytest.mark.parametrize('mode', cc.KEY_MODES)
def test_lengths_in_one_cluster_under_every_key_order(mixed, mode):
    idx, lab = mixed
    csr = idx.csr
    assert idx.long is not None and idx.ctx.n_reads > csr.n_reads
    rev = (np.random.default_rng(3).integers(0, 2, csr.n_intervals).astype(np.uint8), None)[mode == 'equal']
    want = check(idx, lab, cc.keys_of(csr, mode), rev)
    # every clustered read of L intervals gives L - 1 observations; the long read left alone gives none
    assert int(want['n_obs'].sum()) == sum(n - 1 for k, n in enumerate(LENS) if k != ALONE)


def test_rev_in_the_second_chunk_only(mixed):
    idx, lab = mixed
    rev = (cc.place(idx.csr) >= 64).astype(np.uint8)
    assert rev.sum() > 4000
    key = cc.keys_of(idx.csr, 'shuffled')
    want = check(idx, lab, key, rev)
    plain = jr.junctions_of_csr(idx.csr, lab, key, None)
    assert any(not np.array_equal(want[k], plain[k]) for k in NAMES if want[k].shape == plain[k].shape) or \
        want['n_obs'].shape != plain['n_obs'].shape


def test_no_clusters_and_a_cluster_of_short_reads_only(mixed):
    idx, _ = mixed
    n = idx.csr.n_reads
    key = cc.keys_of(idx.csr, 'ascending')
    got = rows_any(idx.ctx, key, None, np.arange(n, dtype=np.int32))
    assert got['off'].tolist() == [0] and all(got[k].size == 0 for k in jr.COLUMNS)
    lab = np.arange(n, dtype=np.int32)
    short = [cc.rank_of_walk(idx.csr, k) for k in (0, 6, 7, 10)]          # 64, 3, 2 and 17 intervals
    lab[short] = min(short)
    want = check(idx, lab, key)                                       # no long read is clustered: no workgroup kernel
    assert int(want['n_obs'].sum()) == 63 + 2 + 1 + 16


# ------------------------------------------------------------------ 2. single observations
def test_the_observations_at_the_seam_and_at_the_end():
    """A read of 130 pieces in locus 0, but for its pieces 63, 64, 128 and 129 in loci 1, 2, 3 and 4: the junctions
    1R-2L and 3R-4L are seen once each, by the observations of chain ranks 63 and L - 2, with the breakpoints of
    exactly those pieces."""
    walk = [(0, 0)] * 130
    for t, a in ((63, 1), (64, 2), (128, 3), (129, 4)):
        walk[t] = (a, 0)
    c = _lib.Context(0)
    try:
        idx, key, rev = cc.index_of_walks(c, [walk, [(0, 0), (1, 0)]])
        want = check(idx, np.zeros(2, np.int32), key, rev)
        ends = list(zip(want['locus_a'].tolist(), want['side_a'].tolist(), want['locus_b'].tolist(), want['side_b'].tolist()))
        G = cc.GAP
        for (a, b), (ta, tb) in (((1, 2), (63, 64)), ((3, 4), (128, 129))):
            i = ends.index((a, 1, b, 0))
            assert want['n_obs'][i] == 1 and want['n_reads'][i] == 1
            assert want['bp_a_min'][i] == want['bp_a_max'][i] == G * a + 50000 + ta         # piece ta's end
            assert want['bp_b_min'][i] == want['bp_b_max'][i] == G * b + 8 * tb             # piece tb's start
    finally:
        c.close()


def test_a_long_read_observes_one_junction_many_times_and_shares_it_with_a_short_read():
    long_walk = [(t % 2, 0) for t in range(200)]                      # 0 1 0 1 ...: 0R-1L 100 times, 0L-1R 99 times
    c = _lib.Context(0)
    try:
        idx, key, rev = cc.index_of_walks(c, [long_walk, [(2, 0), (3, 0)], [(0, 0), (1, 0)]])
        lab = np.zeros(3, np.int32)
        alone = cc.rank_of_walk(idx.csr, 2)
        other = np.asarray([r for r in range(3) if r != alone])
        lab[other], lab[alone] = other.min(), alone
        want = check(idx, lab, key, rev)                              # the long read and the read in loci 2, 3
        by = {(a, sa, b, sb): (o, r) for a, sa, b, sb, o, r in zip(*(want[k].tolist() for k in jr.COLUMNS[:6]))}
        assert by[(0, 1, 1, 0)] == (100, 1) and by[(0, 0, 1, 1)] == (99, 1)
        want = check(idx, np.zeros(3, np.int32), key, rev)            # with the short read that walks 0 -> 1
        by = {(a, sa, b, sb): (o, r) for a, sa, b, sb, o, r in zip(*(want[k].tolist() for k in jr.COLUMNS[:6]))}
        assert by[(0, 1, 1, 0)] == (101, 2) and by[(0, 0, 1, 1)] == (99, 1)
    finally:
        c.close()


# ------------------------------------------------------------------ 3. contexts without long reads
def test_without_long_reads_the_bytes_are_the_plain_call_s():
    data, csr, cid, nc, kw = fixture_membership('cfg1_1k_x3')
    idx = cluster.build_interval_trees(data)
    try:
        assert idx.long is None
        c = idx.ctx
        rng = np.random.default_rng(2)
        key, rev = rng.integers(-50, 50, csr.n_intervals).astype(np.int32), rng.integers(0, 2, csr.n_intervals).astype(np.uint8)
        cluster.cluster_table(query(idx, data, kw), ctx=c)
        c.cluster_loci()
        plain = dict(zip(NAMES, c.cluster_junctions(key, rev)))
        assert len(plain['n_obs']) > 10
        got = dict(zip(NAMES, c.cluster_junctions_any(key, rev)))
        same_rows(got, plain)
        resident_equals(c, plain)                                     # through the getter, after the _any call
        assert [got[k].tobytes() for k in NAMES] == [plain[k].tobytes() for k in NAMES]
        a = idx.cluster_junctions(np.arange(csr.n_intervals), None)
        b = idx.cluster_junctions_any(np.arange(csr.n_intervals), None)
        assert all(np.array_equal(getattr(a, k), getattr(b, k)) for k in NAMES)
    finally:
        idx.ctx.close()


# ------------------------------------------------------------------ 4. state
def test_state_a_failed_call_and_a_new_loci_call():
    c = _lib.Context(0, profiling=True)
    try:
        idx = cc.index_of_lens(c, (130, 5, 66, 2), seed=8)
        csr, n = idx.csr, idx.csr.n_reads
        key = cc.keys_of(csr, 'shuffled')
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*no cluster table'):
            c.cluster_junctions_any(key)
        lab = np.zeros(n, np.int32)
        c.cluster_table(lab)
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_loci first'):
            c.cluster_junctions_any(key)
        want = check(idx, lab, key)
        assert c.cluster_junctions_timings()['junctions'] > 0
        # two runs give the same bytes
        again = rows_any(c, key, loci=False)
        assert [again[k].tobytes() for k in NAMES] == [want[k].tobytes() for k in NAMES]
        # failed calls keep the rows: a wrong count, NULL keys, a table over the virtual reads
        with pytest.raises(_lib.FslrError, match=f'{INVALID}.*n_intervals'):
            c.cluster_junctions_any(key[:-1])
        nrows = _lib.ctypes.c_int64(-7)
        assert c._L.fslr_cluster_junctions_any(c._h, None, None, csr.n_intervals, _lib.ctypes.byref(nrows)) == _lib.FSLR_ERR_INVALID
        assert nrows.value == -7
        resident_equals(c, want)
        with pytest.raises(_lib.FslrError, match=f'{INVALID}.*more than 64'):      # the plain call still refuses
            c.cluster_junctions(key)
        resident_equals(c, want)
        # a new cluster_loci drops them
        c.cluster_loci()
        assert get_rows(c, 1, len(want['n_obs']))[0] == _lib.FSLR_ERR_STATE
        same_rows(rows_any(c, key, loci=False), want)
        # append_any / remove_any leave a stale table: refused, the rows made before still answer
        keep = np.ones(n, bool)
        keep[cc.rank_of_walk(csr, 1)] = False
        idx.remove_any(keep=keep)
        assert idx.csr.n_reads == n - 1
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_table again'):
            c.cluster_junctions_any(cc.keys_of(idx.csr, 'ascending'))
        resident_equals(c, want)
        lab = np.zeros(n - 1, np.int32)
        check(idx, lab, cc.keys_of(idx.csr, 'descending'))
    finally:
        c.close()


def test_append_any_leaves_a_stale_table():
    data, csr, cid, nc, kw = fixture_membership('longreads_400')
    codes = np.unique(data.qcode)
    late = np.isin(data.qcode, codes[codes.size * 2 // 3:])
    idx = cluster.build_interval_trees(data.select(~late))
    try:
        c = idx.ctx
        assert idx.long is not None
        key = cc.keys_of(idx.csr, 'shuffled')
        want = check(idx, cc.groups_of(idx.csr.n_reads, 5), key)
        assert ((np.diff(idx.csr.read_off) > 64).sum()) > 20
        idx.append_any(data.select(late))
        key = cc.keys_of(idx.csr, 'shuffled')
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_table again'):
            c.cluster_junctions_any(key)
        resident_equals(c, want)
        check(idx, cc.groups_of(idx.csr.n_reads, 5), key)
    finally:
        idx.ctx.close()
