"""Cluster paths for reads of more than 64 intervals (fslr_cluster_paths_any) against tests/paths_ref.py, which states
the contract for lists of any length.  Hand-built inputs of a handful of reads; every comparison is exact, dtypes
included.  The golden fixture with long reads goes through the wrappers and the command line, junctions included."""
import os

import numpy as np
import pandas as pd
import pytest

import chain_any_cases as cc
import fixtures as fx
import junctions_ref as jr
import loci_ref as lr
import paths_ref as pr
from fslr_amd import _lib, cluster
from test_gpu_junctions import bed_inputs, same_rows
from test_gpu_loci import fixture_membership, query, run_cli
from test_gpu_paths import get_rows, resident_equals, same

pytestmark = pytest.mark.gpu

STATE = f'fslr error {_lib.FSLR_ERR_STATE}'
INVALID = f'fslr error {_lib.FSLR_ERR_INVALID}'
LENS = (64, 65, 128, 129, 1000, 4096, 3, 2, 1, 70, 17)
ALONE = 9


def rows_any(c, qkey, rev=None, labels=None, loci=True):
    if labels is not None:
        c.cluster_table(labels)
    if loci:
        c.cluster_loci()
    return dict(zip(pr.NAMES, c.cluster_paths_any(qkey, rev)))


def check(idx, labels, qkey, rev=None):
    want = pr.paths_of_csr(idx.csr, labels, qkey, rev)
    same(rows_any(idx.ctx, qkey, rev, labels), want)
    # the n_reads of a cluster's rows sum to the cluster's size
    cid, nc = lr.cids_of_labels(labels)
    sums = np.add.reduceat(np.append(want['n_reads'], 0).astype(np.int64), want['off'][:-1]) if nc else np.zeros(0, np.int64)
    np.testing.assert_array_equal(sums, np.bincount(cid[cid >= 0], minlength=nc))
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
    assert want['path_of_read'].size == want['flipped'].size == csr.n_reads          # per real read
    alone = cc.rank_of_walk(csr, ALONE)
    assert want['path_of_read'][alone] == -1 and (np.delete(want['path_of_read'], alone) >= 0).all()
    assert sorted(np.diff(want['tok_off']).tolist()) == sorted(n for k, n in enumerate(LENS) if k != ALONE)


def test_a_cluster_of_short_reads_only_and_no_clusters(mixed):
    idx, _ = mixed
    csr, n = idx.csr, idx.csr.n_reads
    key = cc.keys_of(csr, 'shuffled')
    lab = np.arange(n, dtype=np.int32)
    short = [cc.rank_of_walk(csr, k) for k in (0, 6, 7, 8, 10)]       # 64, 3, 2, 1 and 17 intervals
    lab[short] = min(short)
    want = check(idx, lab, key)                                       # no long read is clustered: no workgroup kernel
    assert int(want['n_reads'].sum()) == 5
    got = rows_any(idx.ctx, key, None, np.arange(n, dtype=np.int32))
    assert got['off'].tolist() == [0] and got['tok_off'].tolist() == [0] and (got['path_of_read'] == -1).all()


# ------------------------------------------------------------------ 2. the grouping on long chains
def family():
    """Eight walks on eight loci.  W: 4096 pieces, locus 0 forward first, then loci >= 2, so it is canonical as it
    stands (read backwards it starts with a token >= 4) and so is everything that shares its first piece.
    0, 1: W twice; 2: W but for its last piece; 3: W but for piece 64; 4, 5: W's first 64 and 65 pieces; 6: W read
    from the other strand; 7: a palindrome of 80 pieces."""
    rng = np.random.default_rng(40)
    W = [(0, 0)] + [(int(a), int(v)) for a, v in zip(rng.integers(2, 8, 4095), rng.integers(0, 2, 4095))]
    last, seam = list(W), list(W)
    last[4095] = (2 + (W[4095][0] - 1) % 6, W[4095][1])
    seam[64] = (W[64][0], 1 - W[64][1])
    other = [(a, 1 - v) for a, v in reversed(W)]
    X = W[:40]
    return [W, list(W), last, seam, W[:64], W[:65], other, X + [(a, 1 - v) for a, v in reversed(X)]]


@pytest.fixture(scope='module')
def walks():
    c = _lib.Context(0)
    idx, key, rev = cc.index_of_walks(c, family())
    lab = np.zeros(8, np.int32)
    want = pr.paths_of_csr(idx.csr, lab, key, rev)
    yield idx, key, rev, lab, want
    c.close()


def test_equal_long_reads_last_token_seam_token_prefix_reverse_complement_and_palindrome(walks):
    idx, key, rev, lab, want = walks
    same(rows_any(idx.ctx, key, rev, lab), want)
    r = [cc.rank_of_walk(idx.csr, k) for k in range(8)]
    row, flipped = want['path_of_read'], want['flipped']
    # two equal long reads and the same molecule from the other strand: one row, the smallest rank first
    assert row[r[0]] == row[r[1]] == row[r[6]]
    assert want['n_reads'][row[r[0]]] == 3 and want['first_read'][row[r[0]]] == min(r[0], r[1], r[6])
    assert flipped[r[0]] == flipped[r[1]] == 0 and flipped[r[6]] == 1
    # a difference in the last token only, or in token 64 only, is another row
    assert len({row[r[0]], row[r[2]], row[r[3]]}) == 3 and want['n_reads'][row[r[2]]] == want['n_reads'][row[r[3]]] == 1
    # a proper prefix of 64 before its extension of 65, both before W
    assert row[r[4]] < row[r[5]] < row[r[0]]
    # an even-length palindrome is not flipped
    lo, hi = want['tok_off'][row[r[7]]], want['tok_off'][row[r[7]] + 1]
    t = (want['locus'][lo:hi].astype(np.int64) * 2 + want['rev'][lo:hi]).tolist()
    assert hi - lo == 80 and t == [x ^ 1 for x in reversed(t)] and flipped[r[7]] == 0
    assert int(want['n_reads'].sum()) == 8 and len(want['n_reads']) == 6


@pytest.mark.parametrize('pack', ['1', '2', '8'])
def test_the_tokens_per_key_change_no_byte(walks, monkeypatch, pack):
    idx, key, rev, lab, want = walks
    monkeypatch.setenv('FSLR_PATHS_PACK', pack)
    same(rows_any(idx.ctx, key, rev, lab), want)


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
        plain = dict(zip(pr.NAMES, c.cluster_paths(key, rev)))
        assert len(plain['n_reads']) > 10
        got = dict(zip(pr.NAMES, c.cluster_paths_any(key, rev)))
        same(got, plain)
        resident_equals(c, plain)                                     # through the getter, after the _any call
        assert [got[k].tobytes() for k in pr.NAMES] == [plain[k].tobytes() for k in pr.NAMES]
        a = idx.cluster_paths(np.arange(csr.n_intervals), None)
        b = idx.cluster_paths_any(np.arange(csr.n_intervals), None)
        assert all(np.array_equal(getattr(a, k), getattr(b, k)) for k in pr.NAMES)
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
            c.cluster_paths_any(key)
        lab = np.zeros(n, np.int32)
        c.cluster_table(lab)
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_loci first'):
            c.cluster_paths_any(key)
        want = check(idx, lab, key)
        nc, nr, nt = 1, len(want['n_reads']), len(want['locus'])
        assert c.cluster_paths_timings()['paths'] > 0
        # two runs give the same bytes
        again = rows_any(c, key, loci=False)
        assert [again[k].tobytes() for k in pr.NAMES] == [want[k].tobytes() for k in pr.NAMES]
        # failed calls keep the rows: a wrong count, NULL keys, the plain call's refusal
        with pytest.raises(_lib.FslrError, match=f'{INVALID}.*n_intervals'):
            c.cluster_paths_any(key[:-1])
        cnt = _lib.ctypes.c_int64(-7)
        assert c._L.fslr_cluster_paths_any(c._h, None, None, csr.n_intervals, _lib.ctypes.byref(cnt), None) == _lib.FSLR_ERR_INVALID
        assert cnt.value == -7
        with pytest.raises(_lib.FslrError, match=f'{INVALID}.*more than 64'):
            c.cluster_paths(key)
        resident_equals(c, want)
        # the junction rows and the path rows leave each other alone
        junctions = c.cluster_junctions_any(key)
        resident_equals(c, want)
        # a new cluster_loci drops them
        c.cluster_loci()
        assert get_rows(c, nc, n, nr, nt)[0] == _lib.FSLR_ERR_STATE
        same(rows_any(c, key, loci=False), want)
        assert len(junctions[5]) > 0
        # remove_any leaves a stale table: refused, the rows made before still answer
        keep = np.ones(n, bool)
        keep[cc.rank_of_walk(csr, 1)] = False
        idx.remove_any(keep=keep)
        assert idx.csr.n_reads == n - 1 and idx.long is not None
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_table again'):
            c.cluster_paths_any(cc.keys_of(idx.csr, 'ascending'))
        resident_equals(c, want)
        check(idx, np.zeros(n - 1, np.int32), cc.keys_of(idx.csr, 'descending'))
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
            c.cluster_paths_any(key)
        resident_equals(c, want)
        check(idx, cc.groups_of(idx.csr.n_reads, 5), key)
    finally:
        idx.ctx.close()


# ------------------------------------------------------------------ 5. the golden fixture with long reads
def test_wrappers_and_cli_on_the_long_read_fixture(tmp_path):
    name = 'longreads_400'
    data, csr, _, _, kw = fixture_membership(name)
    qstart, _, rev = bed_inputs(name, data)
    pos = np.asarray(csr.data_pos, np.int64)
    idx = cluster.build_interval_trees(data)
    try:
        assert idx.long is not None and int(idx.long.max()) > 64
        got_j = idx.cluster_junctions_any(qstart, rev, query(idx, data, kw))         # the index's own labels
        cid = idx.ctx.cluster_ids()[0]
        nc = int(cid.max()) + 1
        assert cid.size == csr.n_reads and nc > 10 and ((cid >= 0) & (np.diff(csr.read_off) > 64)).sum() > 10
        got_p = idx.cluster_paths_any(qstart, rev)                                   # the table and the loci rows stand
        loci = lr.loci(csr.read_off, csr.iv_chrom, csr.iv_start, csr.iv_end, cid, nc)
        cols = (csr.read_off, csr.iv_chrom, csr.iv_start, csr.iv_end, cid, nc, qstart[pos], rev[pos], loci)
        same_rows({k: getattr(got_j, k) for k in ('off',) + jr.COLUMNS}, jr.junctions(*cols))
        same({k: getattr(got_p, k) for k in pr.NAMES}, pr.paths(*cols))
        with pytest.raises(ValueError, match='intervals'):
            idx.cluster_paths_any(qstart[:-1])
        with pytest.raises(NotImplementedError, match='more than 64'):                # the plain wrapper still refuses
            idx.cluster_junctions(qstart, rev)
        from fslr_amd import fastcli
        name_of = {v: k for k, v in fastcli.chrom_map(list(pd.unique(fx.input_bed(name)['chrom']))).items()}
        frame = got_j.to_frame()
        for col in ('chrom_a', 'chrom_b'):
            frame[col] = [name_of[c] for c in frame[col].tolist()]
        want_j = frame.to_csv(sep='\t', index=False)
        got_p.loci.chrom = np.asarray([name_of[c] for c in got_p.loci.chrom.tolist()], dtype=object)
        want_p = got_p.to_frame().to_csv(sep='\t', index=False)
    finally:
        idx.ctx.close()
    res = run_cli(name, str(tmp_path), '--cluster-junctions', '--cluster-paths', '--cluster-long-reads')
    assert res.exit_code == 0, (res.output, res.exception)
    assert 'file is written' not in res.output
    assert open(os.path.join(str(tmp_path), 'fx.mappings.cluster_junctions.bed')).read() == want_j
    assert open(os.path.join(str(tmp_path), 'fx.mappings.cluster_paths.bed')).read() == want_p
    assert want_j.count('\n') > 100 and want_p.count('\n') > 50
    for which in ('cluster', 'representative'):
        assert open(os.path.join(str(tmp_path), f'fx.mappings.{which}.bed')).read() == fx.expected_text(name, which), which


def test_cli_flag_changes_nothing_without_long_reads(tmp_path):
    texts = []
    for flags in ((), ('--cluster-long-reads',)):
        tmp = tmp_path / str(len(flags))
        tmp.mkdir()
        res = run_cli('cfg1_1k_x3', str(tmp), '--cluster-junctions', '--cluster-paths', *flags)
        assert res.exit_code == 0, (res.output, res.exception)
        texts.append([open(os.path.join(str(tmp), f'fx.mappings.{w}.bed')).read() for w in ('cluster_junctions', 'cluster_paths')])
    assert texts[0] == texts[1] and all(t.count('\n') > 10 for t in texts[0])
