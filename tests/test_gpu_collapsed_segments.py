"""Collapsed path segments on the device (fslr_cluster_collapsed_segments, fslr_cluster_collapsed_segments_any,
fslr_get_cluster_collapsed_segments) against tests/collapsed_ref.py, which tests/test_collapsed_ref.py pins to
hand-worked cases.  Reads walk chosen loci (chain_any_cases.index_of_walks), so every path row's tokens are known; the
clusters come from host label vectors.  Every comparison is exact, dtypes included."""
import os

import numpy as np
import pandas as pd
import pytest

import chain_any_cases as cc
import collapsed_ref as cl
import containment_cases as cs
import containment_ref as cr
import fixtures as fx
import loci_ref as lr
import paths_ref as pr
import segments_ref as sg
from fslr_amd import _lib, cluster
from test_gpu_junctions import bed_inputs
from test_gpu_loci import fixture_membership, run_cli
from test_gpu_path_containment import SEAM_LENS, labels_of, outer_walk, seam_offsets

pytestmark = pytest.mark.gpu

INVALID = f'fslr error {_lib.FSLR_ERR_INVALID}'
STATE = f'fslr error {_lib.FSLR_ERR_STATE}'
GAPS = cl.NAMES[8:]


def same(got, want, names=cl.NAMES):
    for k in names:
        assert got[k].dtype == want[k].dtype == np.int32, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def blob(got):
    return [got[k].tobytes() for k in cl.NAMES]


def rc(walk):
    """The same molecule read from the other strand."""
    return [(a, 1 - v) for a, v in reversed(walk)]


def ends_near(key, rng):
    return (key.astype(np.int64) + rng.integers(-3, 4, key.size)).astype(np.int32)


def device(c, key, qend=None, rev=None, labels=None, rows=True, call='cluster_collapsed_segments_any'):
    """The eleven columns; with ``rows`` the table's loci, paths and containment are made first."""
    if labels is not None:
        c.cluster_table(labels)
    if rows:
        c.cluster_loci()
        c.cluster_paths_any(key, rev)
        c.cluster_path_containment()
    return dict(zip(cl.NAMES, getattr(c, call)(key, qend)))


def statement(csr, lab, key, qend=None, rev=None):
    p = pr.paths_of_csr(csr, lab, key, rev)
    ct = cr.containment(p)
    return p, ct, cl.collapsed_of_csr(csr, p, ct, key, qend)


def sums(p, ct, want):
    """On the columns ``want`` (the callers give the device's): per maximal row the n_cov of its slots sum to n_reads x length over the rows that collapse to it; no slot holds
    more intervals than collapsed_reads; the slots of the other rows and every last slot's links are 0."""
    lens = np.diff(p['tok_off'])
    row = np.repeat(np.arange(len(lens)), lens)
    to = ct['collapse_to'].astype(np.int64)
    np.testing.assert_array_equal(np.bincount(row, want['n_cov'], minlength=len(lens)).astype(np.int64),
                                  np.bincount(to, p['n_reads'].astype(np.int64) * lens, minlength=len(lens)))
    assert (want['n_cov'] <= ct['collapsed_reads'][row]).all() and (want['n_link'] <= want['n_cov']).all()
    inner = to[row] != row
    assert not any(want[k][inner].any() for k in cl.NAMES)
    last = np.asarray(p['tok_off'][1:], np.int64) - 1
    assert not any(want[k][last].any() for k in ('n_link',) + GAPS)


def used_pairs(ct):
    """(offset, rev) of the pair (A, collapse_to[A]) of every row that collapses onto another."""
    out = []
    for A in np.flatnonzero(ct['collapse_to'] != np.arange(len(ct['collapse_to']))).tolist():
        out.append(cl.row_map(ct, A)[1:])
    return out


def check_walks(c, walks, group, seed=1, keys=None, with_qend=True):
    idx, key, rev = cc.index_of_walks(c, walks)
    if keys is not None:
        key = cc.keys_of(idx.csr, keys)
    lab = labels_of(idx.csr, group)
    qend = ends_near(key, np.random.default_rng(seed)) if with_qend else None
    p, ct, want = statement(idx.csr, lab, key, qend, rev)
    got = device(idx.ctx, key, qend, rev, lab)
    same(got, want)
    sums(p, ct, got)
    return idx, (key, qend, rev, lab), p, ct, want


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ 1. seam lengths
def test_inner_seam_lengths_in_outers_of_65_128_and_4096_tokens(ctx):
    """One cluster per outer length; inner reads of every seam length cut at offset 0, at b - a and across positions
    63 / 64 of the outer, every second one read from the other strand; inner rows of 65 and 129 tokens in the 4096
    outer go through the long kernel and write into a row that is not theirs."""
    rng = np.random.default_rng(7)
    walks, group = [], []
    for g, b in enumerate((65, 128, 4096)):
        W = outer_walk(rng, b)
        walks.append(W), group.append(g)
        cuts = [(a, o) for a in SEAM_LENS for o in seam_offsets(a, b)]
        if b == 4096:
            cuts += [(65, 0), (65, 4031), (129, 3000), (129, 1)]
        for k, (a, o) in enumerate(cuts):
            sub = W[o:o + a]
            walks.append(rc(sub) if k % 2 else sub), group.append(g)
    idx, _, p, ct, want = check_walks(ctx, walks, group)
    assert idx.long is not None
    lens = np.diff(p['tok_off'])
    inner = np.flatnonzero(ct['collapse_to'] != np.arange(len(lens)))
    assert set(SEAM_LENS) | {65, 129} <= set(lens[inner].tolist())
    assert set(lens[ct['collapse_to'][inner]].tolist()) == {65, 128, 4096}
    pairs = used_pairs(ct)
    assert {d for _, d in pairs} == {0, 1}                                  # rev has both values
    assert {0, 63} <= {o for o, _ in pairs} and max(o for o, _ in pairs) >= 4031
    assert set(p['flipped'].tolist()) == {0, 1}
    assert int(want['n_cov'].max()) >= 3 and (want['gap_min'] < want['gap_max']).any()


# ------------------------------------------------------------------ 2. popular rows and the tiers
def test_popular_rows_cross_both_tier_seams_and_moved_seams_give_the_same_bytes(monkeypatch):
    """An outer of four pieces read by 3 reads, its pieces 1..2 by 70 reads, its pieces 2..3 by 5000 and piece 1 alone
    by 5: n_cov = 3, 78, 5073, 5003 and n_link = 3, 73, 5003, 0, so the slots of the LDS tier and of the select tier
    hold fewer links than intervals."""
    for name in ('FSLR_SEGS_SMALL', 'FSLR_SEGS_LDS'):
        monkeypatch.delenv(name, raising=False)
    W = [(0, 0), (2, 0), (3, 1), (4, 0)]
    walks = [W] * 3 + [W[1:3]] * 35 + [rc(W[1:3])] * 35 + [W[2:4]] * 2500 + [rc(W[2:4])] * 2500 + [W[1:2]] * 5
    c = _lib.Context(0)
    try:
        idx, (key, qend, rev, lab), p, ct, want = check_walks(c, walks, [0] * len(walks), seed=2)
        top = int(np.flatnonzero(np.diff(p['tok_off']) == 4)[0])
        s = slice(int(p['tok_off'][top]), int(p['tok_off'][top + 1]))
        assert want['n_cov'][s].tolist() == [3, 78, 5073, 5003] and want['n_link'][s].tolist() == [3, 73, 5003, 0]
        assert (want['gap_min'][s][1:3] < want['gap_med'][s][1:3]).all() and (want['gap_med'][s][1:3] < want['gap_max'][s][1:3]).all()
        blobs = [blob(want)]
        for small, lds in (('64', '4096'), ('1', '2'), ('4', '8'), ('16', '16')):
            monkeypatch.setenv('FSLR_SEGS_SMALL', small)
            monkeypatch.setenv('FSLR_SEGS_LDS', lds)
            got = device(c, key, qend, rows=False)
            same(got, want)
            blobs.append(blob(got))
        assert all(b == blobs[0] for b in blobs)
    finally:
        c.close()


@pytest.mark.parametrize('tiers', [None, ('1', '2')])
def test_a_stream_of_one_value_beside_a_stream_of_two(ctx, monkeypatch, tiers):
    """Cluster 0: an outer of three pieces and its pieces 1..2, read once each: n_cov = 1, 2, 2 and n_link = 1, 2, 0.
    Cluster 1: an outer of three pieces and a one-piece read on its piece 1: n_cov = 1, 2, 1 and n_link = 1, 1, 0, so
    slot 1 selects among two coordinates and takes its one gap as it is; the slots of one interval are written by the
    descriptor pass.  Under (FSLR_SEGS_SMALL, FSLR_SEGS_LDS) = (1, 2) the slots of two go through the LDS tier."""
    for name, v in zip(('FSLR_SEGS_SMALL', 'FSLR_SEGS_LDS'), tiers or (None, None)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)
    A = [(0, 0), (2, 0), (3, 0)]
    B = [(0, 0), (4, 1), (5, 0)]
    _, _, p, ct, want = check_walks(ctx, [A, A[1:3], B, B[1:2]], [0, 0, 1, 1], seed=3)
    tops = np.flatnonzero(np.diff(p['tok_off']) == 3).tolist()
    cov = [want['n_cov'][int(p['tok_off'][r]):int(p['tok_off'][r + 1])].tolist() for r in tops]
    link = [want['n_link'][int(p['tok_off'][r]):int(p['tok_off'][r + 1])].tolist() for r in tops]
    assert sorted(zip(map(tuple, cov), map(tuple, link))) == [((1, 2, 1), (1, 1, 0)), ((1, 2, 2), (1, 2, 0))]
    s = int(p['tok_off'][[r for r, cv in zip(tops, cov) if cv == [1, 2, 1]][0]]) + 1
    assert want['gap_min'][s] == want['gap_med'][s] == want['gap_max'][s] != 0       # k = 1 beside k = 2
    assert want['start_min'][s] < want['start_max'][s]


# ------------------------------------------------------------------ 3. no containment, no query ends
def test_without_containment_the_bytes_are_the_path_segments(ctx):
    """Clusters whose reads all walk one molecule, from either strand, one of 70 pieces among them, and a cluster of
    two rows of equal length: every row is maximal."""
    rng = np.random.default_rng(4)
    walks, group = [], []
    for g in range(6):
        W = outer_walk(rng, int(rng.integers(2, 9)))
        m = int(rng.integers(1, 5))
        walks += [W] * m + [rc(W)]
        group += [g] * (m + 1)
    W = outer_walk(rng, 70)
    walks += [W, rc(W), [(0, 0), (2, 0), (3, 0)], [(0, 0), (2, 1), (4, 0)]]
    group += [6, 6, 7, 7]
    idx, (key, qend, rev, lab), p, ct, want = check_walks(ctx, walks, group, seed=5)
    assert len(ct['outer']) == 0 and (ct['collapse_to'] == np.arange(len(p['n_reads']))).all()
    seg = dict(zip(sg.NAMES, idx.ctx.cluster_path_segments_any(key, qend)))
    got = device(idx.ctx, key, qend, rows=False)
    for k in sg.NAMES:
        assert got[k].tobytes() == seg[k].tobytes(), k
    np.testing.assert_array_equal(got['n_cov'], np.repeat(p['n_reads'], np.diff(p['tok_off'])))
    assert (p['n_reads'] >= 2).any() and int(np.diff(p['tok_off']).max()) == 70


def test_without_query_ends_the_gaps_are_0_and_n_link_is_filled(ctx):
    rng = np.random.default_rng(6)
    W = outer_walk(rng, 70)
    walks = [W, W, W[3:20], rc(W[60:]), W[:5], rc(W[10:12])]
    idx, (key, _, rev, lab), p, ct, want = check_walks(ctx, walks, [0] * len(walks), with_qend=False)
    assert not any(want[k].any() for k in GAPS) and int(want['n_link'].max()) >= 3
    with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_set_profiling'):      # a successful call, no profiling context
        idx.ctx.cluster_collapsed_segments_timings()
    with_ends = device(idx.ctx, key, ends_near(key, rng), rows=False)
    np.testing.assert_array_equal(with_ends['n_link'], want['n_link'])
    assert with_ends['gap_med'].any()


# ------------------------------------------------------------------ 4. chunk-seam keys
@pytest.mark.parametrize('mode', ['equal', 'seam_equal', 'seam_extremes'])
def test_chunk_seam_keys_on_a_long_read_that_collapses(ctx, mode):
    """Every piece lies on one locus, forward, so the token chains do not depend on the keys: a read of 70 pieces
    collapses onto the row of 100 whatever the key order, and the keys decide which interval lands in which slot."""
    t = [(5, 0)]
    walks = [t * 100, t * 100, t * 70, t * 66, t * 3]
    idx, _, p, ct, want = check_walks(ctx, walks, [0] * len(walks), seed=8, keys=mode)
    assert idx.long is not None and np.diff(p['tok_off']).tolist() == [3, 66, 70, 100]
    assert ct['collapse_to'].tolist() == [3, 3, 3, 3]
    s = int(p['tok_off'][3])
    assert want['n_cov'][s:].tolist() == [5] * 3 + [4] * 63 + [3] * 4 + [2] * 30


# ------------------------------------------------------------------ 5. the golden fixtures with truncated reads
def names_of(name, data):
    from fslr_amd import fastcli
    name_of = {v: k for k, v in fastcli.chrom_map(list(pd.unique(fx.input_bed(name)['chrom']))).items()}
    return [name_of[v] for v in np.unique(data.chrom).tolist()]


HEADER = ('chrom\tstart\tend\tcluster\tpath\tpiece\tstrand\tn_cov\tstart_min\tstart_max\tend_min\tend_max\tgap_min\tgap\tgap_max'
          '\tn_link\tcollapsed_reads\n')


def expected_text(p, ct, want, loci, dense_names):
    """The file of --cluster-collapsed-segments from the plain statement alone."""
    lines = []
    for c in range(len(p['off']) - 1):
        for i in range(int(p['off'][c]), int(p['off'][c + 1])):
            if int(ct['collapse_to'][i]) != i:
                continue
            for j, s in enumerate(range(int(p['tok_off'][i]), int(p['tok_off'][i + 1]))):
                lines.append((dense_names[loci['chrom'][p['locus'][s]]], want['start_med'][s], want['end_med'][s], c,
                              i - int(p['off'][c]), j, '-' if p['rev'][s] else '+', want['n_cov'][s], want['start_min'][s],
                              want['start_max'][s], want['end_min'][s], want['end_max'][s], want['gap_min'][s],
                              want['gap_med'][s], want['gap_max'][s], want['n_link'][s], ct['collapsed_reads'][i]))
    return HEADER + ''.join('\t'.join(map(str, r)) + '\n' for r in lines)


@pytest.mark.parametrize('name, n_pairs, n_long', [('cfg1_1k_x3', 348, 0), ('longreads_400', 140, 79)])
def test_truncated_fixture_through_the_wrapper_and_the_writer(tmp_path, name, n_pairs, n_long):
    from fslr_amd.main import write_cluster_collapsed_segments
    from fslr_amd import fastcli
    data, qstart, rev, cid_of_code = cs.truncated_fixture(name)
    bed = fx.input_bed(name)
    qend = bed['qend'].to_numpy()[np.asarray(data.index, np.int64)]
    path = os.path.join(str(tmp_path), 'fx.mappings.bed')
    with open(path, 'w') as fh:
        fh.write(fx.input_bed_text(name))
    idx = cluster.build_interval_trees(data)
    try:
        csr = idx.csr
        pos = np.asarray(csr.data_pos, np.int64)
        lab = cs.labels_for(csr, cid_of_code)
        cid, nc = lr.cids_of_labels(lab)
        loci = lr.loci(csr.read_off, csr.iv_chrom, csr.iv_start, csr.iv_end, cid, nc)
        p = pr.paths(csr.read_off, csr.iv_chrom, csr.iv_start, csr.iv_end, cid, nc, qstart[pos], rev[pos], loci)
        ct = cr.containment(p)
        want = cl.collapsed_of_csr(csr, p, ct, qstart[pos], qend[pos])
        lens = np.diff(p['tok_off'])
        inner = np.repeat(np.arange(len(lens)), np.diff(ct['coff']))
        assert len(ct['outer']) == n_pairs and (int((lens[inner] > 64).sum()) > 10) == (n_long > 0)
        assert (idx.long is not None) == (name == 'longreads_400')
        got = idx.cluster_collapsed_segments_any(qstart, qend, rev, lab)
        assert isinstance(got, cluster.ClusterCollapsedSegments) and isinstance(got.containment, cluster.ClusterPathContainment)
        same(dict(zip(cl.NAMES, got.columns())), want)
        sums(p, ct, dict(zip(cl.NAMES, got.columns())))
        assert {d for _, d in used_pairs(ct)} == {0, 1} and int(want['n_cov'].max()) >= 3
        again = idx.cluster_collapsed_segments_any(qstart, qend, rev)                 # on the resident path rows
        assert again.paths is got.paths
        same(dict(zip(cl.NAMES, again.columns())), want)
        if idx.long is None:                                                           # the plain call: the same bytes
            plain = idx.cluster_collapsed_segments(qstart, qend, rev)
            assert blob(dict(zip(cl.NAMES, plain.columns()))) == blob(want)
            raw = dict(zip(cl.NAMES, idx.ctx.cluster_collapsed_segments(qstart[pos].astype(np.int32), qend[pos].astype(np.int32))))
            assert blob(raw) == blob(want)
        else:
            with pytest.raises(NotImplementedError, match='more than 64'):
                idx.cluster_collapsed_segments(qstart, qend, rev)
            with pytest.raises(_lib.FslrError, match=f'{INVALID}.*more than 64'):
                idx.ctx.cluster_collapsed_segments(qstart[pos].astype(np.int32))
        frame = got.to_frame()
        keep = (ct['collapse_to'] == np.arange(len(lens)))[np.repeat(np.arange(len(lens)), lens)]
        np.testing.assert_array_equal(frame['n_cov'].to_numpy(), want['n_cov'][keep])
        out = os.path.join(str(tmp_path), 'out.bed')
        cmap = fastcli.chrom_map(list(pd.unique(bed['chrom'])))
        assert write_cluster_collapsed_segments(out, path, idx, lab, cmap)
        assert open(out).read() == expected_text(p, ct, want, loci, names_of(name, data))
    finally:
        idx.ctx.close()


@pytest.mark.parametrize('io_flag', ['--native-io', '--pandas-io'])
@pytest.mark.parametrize('name', ['cfg1_1k_x3', 'longreads_400'])
def test_cli_in_both_io_modes(tmp_path, name, io_flag):
    """The flag end to end on the fixtures as they are (their own clusters hold no contained path, so this covers the
    plumbing, reads of more than 64 intervals included; the truncated reads go through the writer above)."""
    data, csr, cid, nc, kw = fixture_membership(name)
    qstart, _, rev = bed_inputs(name, data)
    qend = fx.input_bed(name)['qend'].to_numpy()[np.asarray(data.index, np.int64)]
    pos = np.asarray(csr.data_pos, np.int64)
    loci = lr.loci(csr.read_off, csr.iv_chrom, csr.iv_start, csr.iv_end, cid, nc)
    p = pr.paths(csr.read_off, csr.iv_chrom, csr.iv_start, csr.iv_end, cid, nc, qstart[pos], rev[pos], loci)
    ct = cr.containment(p)
    want = cl.collapsed_of_csr(csr, p, ct, qstart[pos], qend[pos])
    res = run_cli(name, str(tmp_path), io_flag, '--cluster-collapsed-segments')
    assert res.exit_code == 0, (res.output, res.exception)
    text = open(os.path.join(str(tmp_path), 'fx.mappings.cluster_collapsed_segments.bed')).read()
    assert text == expected_text(p, ct, want, loci, names_of(name, data)) and text.count('\n') > 10
    for which in ('cluster', 'representative'):
        assert open(os.path.join(str(tmp_path), f'fx.mappings.{which}.bed')).read() == fx.expected_text(name, which), which


def test_cli_refuses_several_gpus(tmp_path):
    res = run_cli('cfg1_1k_x3', str(tmp_path), '--cluster-collapsed-segments', '--gpus=2')
    assert res.exit_code == 2 and '--gpus 1' in res.output
    assert sorted(os.listdir(str(tmp_path))) == ['fx.bwa_dodi.bam', 'fx.mappings.bed']


# ------------------------------------------------------------------ 6. state
def get_rows(c, nt, token_capacity, fill=-7):
    outs = [np.full(max(nt, 1), fill, np.int32) for _ in range(2)] + [np.full(3 * max(nt, 1), fill, np.int32) for _ in range(3)]
    return c._L.fslr_get_cluster_collapsed_segments(c._h, *[_lib._ptr(a) for a in outs], token_capacity), outs


def resident_equals(c, want):
    nt = len(want['n_cov'])
    rc_, outs = get_rows(c, nt, nt)
    assert rc_ == _lib.FSLR_OK
    got = {'n_cov': outs[0], 'n_link': outs[1]}
    got.update({f'{kind}_{w}': o[i * nt:(i + 1) * nt] for kind, o in zip(('start', 'end', 'gap'), outs[2:])
                for i, w in enumerate(('min', 'med', 'max'))})
    same(got, want)


def test_state_drops_failed_calls_capacities_two_runs_and_the_timings_call():
    c = _lib.Context(0, profiling=True)
    try:
        rng = np.random.default_rng(12)
        X = outer_walk(rng, 70)
        walks = [X, X[3:20], rc(X[60:]), X[:5], X[10:12]]
        idx, key, rev = cc.index_of_walks(c, walks)
        qend = ends_near(key, rng)
        lab = np.zeros(len(walks), np.int32)
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*no cluster table'):
            c.cluster_collapsed_segments_any(key, qend)
        c.cluster_table(lab)
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_loci first'):
            c.cluster_collapsed_segments_any(key, qend)
        c.cluster_loci()
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_paths first'):
            c.cluster_collapsed_segments_any(key, qend)
        c.cluster_paths_any(key, rev)
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_path_containment first'):
            c.cluster_collapsed_segments_any(key, qend)
        assert get_rows(c, 0, 0)[0] == _lib.FSLR_ERR_STATE                    # a failed call installed nothing
        with pytest.raises(_lib.FslrError, match=STATE):
            c.cluster_collapsed_segments_timings()
        p, ct, want = statement(idx.csr, lab, key, qend, rev)
        nt = len(want['n_cov'])
        c.cluster_path_containment()
        got = device(c, key, qend, rows=False)
        same(got, want)
        assert c.cluster_collapsed_segments_timings()['collapsed'] > 0
        assert blob(device(c, key, qend, rows=False)) == blob(want)          # two runs give the same bytes
        resident_equals(c, want)
        # failed calls keep the rows: the plain call on virtual reads, a wrong count, NULL keys
        with pytest.raises(_lib.FslrError, match=f'{INVALID}.*more than 64'):
            c.cluster_collapsed_segments(key, qend)
        resident_equals(c, want)
        with pytest.raises(_lib.FslrError, match=f'{INVALID}.*n_intervals'):
            c.cluster_collapsed_segments_any(key[:-1], qend[:-1])
        resident_equals(c, want)
        cnt = _lib.ctypes.c_int64(-7)
        assert c._L.fslr_cluster_collapsed_segments_any(c._h, None, _lib._ptr(qend), idx.csr.n_intervals, _lib.ctypes.byref(cnt)) == \
            _lib.FSLR_ERR_INVALID
        assert cnt.value == -7 and 'NULL' in c._L.fslr_last_error(c._h).decode()
        resident_equals(c, want)
        # a small capacity is refused and nothing is written; NULL outputs are skipped
        rc_, outs = get_rows(c, nt, nt - 1)
        assert rc_ == _lib.FSLR_ERR_INVALID and b'capacity' in c._L.fslr_last_error(c._h)
        assert all((o == -7).all() for o in outs)
        n_link = np.full(nt, -7, np.int32)
        assert c._L.fslr_get_cluster_collapsed_segments(c._h, None, _lib._ptr(n_link), None, None, None, nt) == _lib.FSLR_OK
        np.testing.assert_array_equal(n_link, want['n_link'])
        # a new containment, new path rows and a new table each drop the rows
        c.cluster_path_containment()
        assert get_rows(c, nt, nt)[0] == _lib.FSLR_ERR_STATE
        same(device(c, key, qend, rows=False), want)
        c.cluster_paths_any(key, rev)
        assert get_rows(c, nt, nt)[0] == _lib.FSLR_ERR_STATE
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_path_containment first'):
            c.cluster_collapsed_segments_any(key, qend)
        c.cluster_path_containment()
        same(device(c, key, qend, rows=False), want)
        c.cluster_table(lab)
        assert get_rows(c, nt, nt)[0] == _lib.FSLR_ERR_STATE
        same(device(c, key, qend, rev), want)
        # the path rows, their segments and the containment rows are left alone
        seg = sg.segments(idx.csr.read_off, idx.csr.iv_start, idx.csr.iv_end, p, key, qend)
        got_seg = dict(zip(sg.NAMES, c.cluster_path_segments_any(key, qend)))
        same(device(c, key, qend, rows=False), want)
        for k in sg.NAMES:
            np.testing.assert_array_equal(got_seg[k], seg[k], err_msg=k)
        resident_equals(c, want)
    finally:
        c.close()
