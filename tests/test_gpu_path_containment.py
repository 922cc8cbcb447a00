"""Path containment on the device (fslr_cluster_path_containment, fslr_get_cluster_path_containment) against
tests/containment_ref.py, which tests/test_containment_ref.py pins to hand-worked cases.  Reads walk chosen loci
(chain_any_cases.index_of_walks), so every path row's tokens are known; the clusters come from host label vectors.
Every comparison is exact, dtypes included."""
import os

import numpy as np
import pytest

import chain_any_cases as cc
import containment_cases as cs
import containment_ref as cr
import fixtures as fx
import loci_ref as lr
import paths_ref as pr
import search_ref as sr
from fslr_amd import _lib, cluster
from test_gpu_junctions import bed_inputs, build, groups_of, index_of, keys_of
from test_gpu_loci import fixture_membership, run_cli
from test_gpu_paths import resident_equals as path_rows_equal

pytestmark = pytest.mark.gpu

INVALID = f'fslr error {_lib.FSLR_ERR_INVALID}'
STATE = f'fslr error {_lib.FSLR_ERR_STATE}'
SEAM_LENS = (1, 2, 15, 16, 17, 32, 33, 63, 64)


def same(got, want, names=cr.NAMES):
    for k in names:
        assert got[k].dtype == want[k].dtype, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def labels_of(csr, group):
    """Min-rank labels: walk k (its place in the list given to index_of_walks) lies in cluster ``group[k]``; a group
    of one read stays alone."""
    g = np.asarray(group, np.int64)[np.asarray(csr.read_qcode)]
    lab = np.arange(csr.n_reads, dtype=np.int32)
    for gid in np.unique(g).tolist():
        m = np.flatnonzero(g == gid)
        if m.size >= 2:
            lab[m] = m.min()
    return lab


def device(c, key, rev, labels=None, loci=True, paths=True, call='cluster_paths_any'):
    if labels is not None:
        c.cluster_table(labels)
    if loci:
        c.cluster_loci()
    p = dict(zip(pr.NAMES, getattr(c, call)(key, rev))) if paths else None
    return p, dict(zip(cr.NAMES, c.cluster_path_containment()))


def check_walks(c, walks, group):
    """The device's rows for ``walks`` in the clusters ``group`` against the statement; returns (paths, rows)."""
    idx, key, rev = cc.index_of_walks(c, walks)
    lab = labels_of(idx.csr, group)
    want_p = pr.paths_of_csr(idx.csr, lab, key, rev)
    got_p, got = device(c, key, rev, lab)
    for k in pr.NAMES:
        np.testing.assert_array_equal(got_p[k], want_p[k], err_msg=k)
    want = cr.containment(want_p)
    same(got, want)
    cluster_sums(want_p, want, lab)
    return want_p, want


def cluster_sums(p, res, lab):
    """The collapsed_reads of a cluster's rows sum to the cluster's size; every pair lies in one cluster."""
    cid, nc = lr.cids_of_labels(lab)
    of_row = np.repeat(np.arange(nc), np.diff(p['off']))
    np.testing.assert_array_equal(np.bincount(of_row, res['collapsed_reads'], minlength=nc).astype(np.int64),
                                  np.bincount(cid[cid >= 0], minlength=nc))
    inner = np.repeat(np.arange(len(res['coff']) - 1), np.diff(res['coff']))
    assert (of_row[inner] == of_row[res['outer']]).all()
    assert (np.diff(p['tok_off'])[inner] < np.diff(p['tok_off'])[res['outer']]).all()


def outer_walk(rng, b):
    """A walk of ``b`` pieces that is canonical as it stands: locus 0 forward first, then loci 2..7 (read backwards
    it starts with a token >= 4)."""
    return [(0, 0)] + [(int(a), int(v)) for a, v in zip(rng.integers(2, 8, b - 1), rng.integers(0, 2, b - 1))]


def seam_offsets(a, b):
    """Offset 0, offset b - a, and one that straddles positions 63 / 64 of the outer."""
    return sorted({0, b - a, min(max(64 - (a + 1) // 2, 0), b - a), min(63, b - a)})


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ 1. inner-length seams
def test_inner_lengths_alone_in_a_wavefront(ctx):
    """Clusters of four rows each: an outer of 65, 128 or 4096 tokens (the workgroup kernel's), one inner of a seam
    length cut from it, and two one-token rows of loci the outer never visits.  The rows of a cluster fill one
    wavefront's quad, so the inner decides its lane-group width alone."""
    rng = np.random.default_rng(7)
    walks, group = [], []
    for b in (65, 128, 4096):
        for a in SEAM_LENS:
            for o in seam_offsets(a, b):
                W = outer_walk(rng, b)
                walks += [W, W[o:o + a], [(1, 0)], [(8, 0)]]
                group += [len(group) // 4] * 4
    p, res = check_walks(ctx, walks, group)
    assert (np.diff(p['off']) == 4).all() and len(p['off']) - 1 == len(walks) // 4
    # per cluster: the inner lies in the outer
    assert (np.bincount(np.repeat(np.arange(len(p['off']) - 1), 4), res['n_inner']) >= 1).all()
    assert int(res['rev'].sum()) > 0 and int((res['rev'] == 0).sum()) > 0     # cut pieces are stored in either direction


def test_inner_lengths_mixed_four_to_a_wavefront(ctx):
    """One cluster per outer length with every seam length at every offset: consecutive rows of mixed lengths share
    wavefronts, inner rows contain one another, and the 4096-token outer is reached at offset 0, at b - a and
    across positions 63 / 64."""
    rng = np.random.default_rng(8)
    walks, group = [], []
    for g, b in enumerate((65, 128, 4096)):
        W = outer_walk(rng, b)
        walks.append(W), group.append(g)
        for a in SEAM_LENS:
            for o in seam_offsets(a, b):
                walks.append(W[o:o + a]), group.append(g)
    p, res = check_walks(ctx, walks, group)
    lens = np.diff(p['tok_off'])
    inner = np.repeat(np.arange(len(lens)), np.diff(res['coff']))
    big = lens[res['outer']] == 4096
    assert set(SEAM_LENS) <= set(lens[inner[big]].tolist())
    assert {0, 63}.issubset(set(res['offset'][big].tolist())) and int(res['offset'][big].max()) >= 4096 - 64


# ------------------------------------------------------------------ 2. workgroup-tier inners
def other_locus(piece):
    """The piece on another of the loci 2..7."""
    return (2 + (piece[0] - 1) % 6, piece[1])


def test_workgroup_tier_inners_and_single_token_mismatches(ctx):
    """Inner rows of 65, 128, 129, 1000 and 4095 tokens cut from a 4096-token outer, and beside each a copy that
    differs in its last token only, in its first only and in token 64 only: those give no pair."""
    rng = np.random.default_rng(9)
    W = outer_walk(rng, 4096)
    walks, broken = [W], []
    for a, o in ((65, 0), (65, 4031), (128, 1), (129, 3000), (1000, 17), (4095, 1)):
        sub = W[o:o + a]
        walks.append(sub)
        for at in (a - 1, 0, 64):
            bad = list(sub)
            bad[at] = other_locus(bad[at])
            broken.append(len(walks))
            walks.append(bad)
    idx, key, rev = cc.index_of_walks(ctx, walks)
    lab = np.zeros(len(walks), np.int32)
    want_p = pr.paths_of_csr(idx.csr, lab, key, rev)
    got_p, got = device(idx.ctx, key, rev, lab)
    want = cr.containment(want_p)
    same(got, want)
    cluster_sums(want_p, want, lab)
    lens = np.diff(want_p['tok_off'])
    top = int(np.flatnonzero(lens == 4096)[0])
    inner = np.repeat(np.arange(len(lens)), np.diff(want['coff']))
    assert sorted(set(lens[inner[want['outer'] == top]].tolist())) == [65, 128, 129, 1000, 4095]
    for k in broken:                                 # a single differing token: the row does not lie in the outer
        row = want_p['path_of_read'][cc.rank_of_walk(idx.csr, k)]
        assert top not in want['outer'][want['coff'][row]:want['coff'][row + 1]].tolist()


# ------------------------------------------------------------------ 3. direction and counting
def test_direction_palindrome_and_occurrence_counts(ctx):
    same_tok = [(5, 0)]
    clusters = [
        [[(0, 0), (1, 0), (4, 1), (3, 1), (2, 1)], [(2, 0), (3, 0), (4, 0)]],              # reverse only
        [[(0, 0), (3, 1), (2, 1), (2, 0), (3, 0)], [(2, 0), (3, 0)]],                      # reverse at 1, forward at 3
        [[(0, 0), (2, 0), (3, 0), (3, 1), (2, 1)], [(2, 0), (3, 0)]],                      # forward at 1, reverse at 3
        [[(0, 0), (1, 0), (1, 1), (3, 0)], [(1, 0), (1, 1)]],                              # a palindromic inner
        [same_tok * 4096, same_tok, same_tok * 100],                                       # one repeated token
    ]
    walks = [w for cl in clusters for w in cl]
    group = [g for g, cl in enumerate(clusters) for _ in cl]
    p, res = check_walks(ctx, walks, group)
    inner = np.repeat(np.arange(len(res['coff']) - 1), np.diff(res['coff']))
    of_row = np.repeat(np.arange(len(clusters)), np.diff(p['off']))
    rows = lambda g: [(int(o), int(d), int(k)) for o, d, k in
                      zip(res['offset'][of_row[inner] == g], res['rev'][of_row[inner] == g], res['n_occ'][of_row[inner] == g])]
    assert rows(0) == [(2, 1, 1)]
    assert rows(1) == [(1, 1, 2)] and rows(2) == [(1, 0, 2)]
    assert rows(3) == [(1, 0, 1)]
    # rows of cluster 4 ascend: (t), (t x 100), (t x 4096); pairs (1 in 100), (1 in 4096), (100 in 4096)
    assert rows(4) == [(0, 0, 100), (0, 0, 4096), (0, 0, 3997)]


# ------------------------------------------------------------------ 4. the quadratic anchor case
def test_300_rows_that_start_with_the_same_token(ctx):
    """Every row of the cluster starts with locus 0 forward, so every forward probe visits every row; the rows are
    prefixes of a few walks on three loci, so short rows lie inside many longer ones."""
    rng = np.random.default_rng(10)
    walks = []
    for _ in range(14):
        X = [(0, 0)] + [(int(a), int(v)) for a, v in zip(rng.integers(1, 4, 29), rng.integers(0, 2, 29))]
        walks += [X[:n] for n in range(1, 31)]
    walks.append([(2, 0), (3, 1)])                   # and one row that starts elsewhere
    p, res = check_walks(ctx, walks, [0] * len(walks))
    n_rows = len(p['n_reads'])
    assert n_rows >= 300 and len(res['outer']) > 2000
    inner = np.repeat(np.arange(n_rows), np.diff(res['coff']))
    have = set(zip(inner.tolist(), res['outer'].tolist()))
    outers = {}
    for a, b in have:
        outers.setdefault(a, []).append(b)
    assert all((a, c) in have for a, b in have for c in outers.get(b, ()))       # transitive
    maximal = np.diff(res['coff']) == 0
    assert maximal[res['collapse_to']].all() and (res['collapsed_reads'][~maximal] == 0).all()


# ------------------------------------------------------------------ 5. no pairs
def test_rows_of_equal_length_one_row_clusters_and_no_clusters(ctx):
    idx = build(ctx, [5] * 12 + [1] * 8, seed=3)
    n = idx.csr.n_reads
    rng = np.random.default_rng(2)
    key = keys_of(idx.csr, 'random', rng)
    lab = groups_of(n, 4)                            # clusters of reads of one length: rows of equal length only
    want_p = pr.paths_of_csr(idx.csr, lab, key)
    got_p, got = device(idx.ctx, key, None, lab, call='cluster_paths')
    want = cr.containment(want_p)
    same(got, want)
    assert len(want['outer']) == 0 and want['coff'].tolist() == [0] * (len(want_p['n_reads']) + 1)
    np.testing.assert_array_equal(got['collapse_to'], np.arange(len(want_p['n_reads'])))
    np.testing.assert_array_equal(got['collapsed_reads'], want_p['n_reads'])
    # every read twice: each cluster has one row
    reads = [[(0, 1000 * r + 7 * t, 1000 * r + 7 * t + 5) for t in range(3)] for r in range(6)]
    idx = index_of(ctx, reads + reads)
    lab = (np.arange(12, dtype=np.int32) // 2) * 2
    key = keys_of(idx.csr, 'ascending', None)
    want_p = pr.paths_of_csr(idx.csr, lab, key)
    assert np.diff(want_p['off']).tolist() == [1] * 6
    got_p, got = device(idx.ctx, key, None, lab, call='cluster_paths')
    same(got, cr.containment(want_p))
    assert got['collapsed_reads'].tolist() == [2] * 6 and got['n_inner'].tolist() == [0] * 6
    # no clusters: no path rows, empty outputs
    got_p, got = device(idx.ctx, key, None, np.arange(12, dtype=np.int32))
    assert got['coff'].tolist() == [0] and all(got[k].size == 0 for k in cr.NAMES[1:])
    same(got, cr.containment(got_p))


# ------------------------------------------------------------------ 6. sort-bit seams
@pytest.mark.parametrize('n_rows', [15, 16, 17, 32, 33, 64, 65])
def test_row_counts_around_a_power_of_two(ctx, n_rows):
    """The occurrences are sorted on 2 * ceil(log2 n_rows) bits.  The prefixes of one walk and the walk without its
    first piece give n_rows rows: the last row is an inner one and the longest prefix the outer of every other, so
    the largest row indices are in a key on both sides."""
    rng = np.random.default_rng(n_rows)
    m = n_rows - 1
    X = [(0, 0)] + [(int(a), int(v)) for a, v in zip(rng.integers(1, 6, m - 1), rng.integers(0, 2, m - 1))]
    p, res = check_walks(ctx, [X[:n] for n in range(1, m + 1)] + [X[1:]], [0] * n_rows)
    assert len(p['n_reads']) == n_rows and len(res['outer']) >= m * (m - 1) // 2
    assert int(res['outer'].max()) == m - 1 and int(np.flatnonzero(np.diff(res['coff']))[-1]) == n_rows - 1


# ------------------------------------------------------------------ 7. long reads and contexts without them
def pair_kinds(p, res):
    """What the pairs of a result cover: (pairs, reverse ones, offsets above 0, inner rows of more than 64 tokens)."""
    lens = np.diff(p['tok_off'])
    inner = np.repeat(np.arange(len(lens)), np.diff(res['coff']))
    return len(res['outer']), int(res['rev'].sum()), int((res['offset'] > 0).sum()), int((lens[inner] > 64).sum())


def test_the_long_read_fixture_with_truncated_reads_through_the_wrapper():
    """The fixture's own clusters hold no contained path, so every second clustered read loses an end piece
    (containment_cases.truncated_fixture): pairs in both directions, at offset 0 and above, inner rows of more than
    64 tokens among them."""
    data, qstart, rev, cid_of_code = cs.truncated_fixture('longreads_400')
    idx = cluster.build_interval_trees(data)
    try:
        csr = idx.csr
        pos = np.asarray(csr.data_pos, np.int64)
        lab = cs.labels_for(csr, cid_of_code)
        assert idx.long is not None and int(idx.long.max()) > 64
        got = idx.cluster_path_containment(qstart, rev, lab)
        assert isinstance(got, cluster.ClusterPathContainment)
        want_p = pr.paths_of_csr(csr, lab, qstart[pos], rev[pos])
        want = cr.containment(want_p)
        same({k: getattr(got, k) for k in cr.NAMES}, want)
        n_pairs, n_rev, n_off, n_long = pair_kinds(want_p, want)
        assert n_pairs > 100 and 0 < n_rev < n_pairs and 0 < n_off < n_pairs and n_long > 10
        assert len(got.paths) == len(want_p['n_reads'])
        # the same arguments again: the resident path rows are reused, the bytes are the same
        paths = got.paths
        again = idx.cluster_path_containment(qstart, rev)
        assert again.paths is paths
        same({k: getattr(again, k) for k in cr.NAMES}, want)
        # the frames
        f = got.to_frame()
        inner = np.repeat(np.arange(len(want_p['n_reads'])), np.diff(want['coff']))
        assert len(f) == n_pairs
        np.testing.assert_array_equal(f['inner'].to_numpy(), inner)
        np.testing.assert_array_equal(f['outer'].to_numpy(), want['outer'])
        np.testing.assert_array_equal(f['rev'].to_numpy(), want['rev'])
        np.testing.assert_array_equal(f['cluster'].to_numpy(), np.repeat(np.arange(len(want_p['off']) - 1), np.diff(want_p['off']))[inner])
        g = got.paths_frame()
        np.testing.assert_array_equal(g['maximal'].to_numpy(), np.diff(want['coff']) == 0)
        np.testing.assert_array_equal(g['collapse_to'].to_numpy(), want['collapse_to'])
        assert (g['collapse_to'].to_numpy() != g['row'].to_numpy()).sum() == (np.diff(want['coff']) > 0).sum() > 100
    finally:
        idx.ctx.close()


def test_without_long_reads_cluster_paths_and_cluster_paths_any_give_the_same_bytes():
    data, qstart, rev, cid_of_code = cs.truncated_fixture('cfg1_1k_x3')
    idx = cluster.build_interval_trees(data)
    try:
        assert idx.long is None
        c, csr = idx.ctx, idx.csr
        pos = np.asarray(csr.data_pos, np.int64)
        key, rv = qstart[pos].astype(np.int32), rev[pos]
        lab = cs.labels_for(csr, cid_of_code)
        p_plain, plain = device(c, key, rv, lab, call='cluster_paths')
        p_any, got = device(c, key, rv, loci=False, call='cluster_paths_any')
        assert [got[k].tobytes() for k in cr.NAMES] == [plain[k].tobytes() for k in cr.NAMES]
        want_p = pr.paths_of_csr(csr, lab, key, rv)
        want = cr.containment(want_p)
        same(got, want)
        n_pairs, n_rev, n_off, _ = pair_kinds(want_p, want)
        assert n_pairs > 100 and 0 < n_rev < n_pairs and 0 < n_off < n_pairs
    finally:
        idx.ctx.close()


# ------------------------------------------------------------------ 8. state
def get_rows(c, n_rows, n_pairs, row_capacity, pair_capacity, fill=-7):
    wide = [np.full(n_rows + 1, fill, np.int64), np.full(n_rows, fill, np.int64), np.full(n_rows, fill, np.int64)]
    ints = [np.full(k, fill, np.int32) for k in (n_pairs, n_pairs, n_pairs, n_rows, n_rows)]
    byts = np.full(n_pairs, 249, np.uint8)
    coff, support, collapsed = wide
    outer, offset, n_occ, n_inner, collapse_to = ints
    rc = c._L.fslr_get_cluster_path_containment(c._h, *[_lib._ptr(a) for a in (coff, outer, offset, byts, n_occ, n_inner, support,
                                                                                 collapse_to, collapsed)], row_capacity, pair_capacity)
    return rc, dict(zip(cr.NAMES, (coff, outer, offset, byts, n_occ, n_inner, support, collapse_to, collapsed)))


def test_state_drops_capacities_two_runs_and_the_timings_call():
    c = _lib.Context(0, profiling=True)
    try:
        rng = np.random.default_rng(12)
        X = outer_walk(rng, 70)
        walks = [X, X[3:20], X[60:], X[:5], X[10:12]]
        idx, key, rev = cc.index_of_walks(c, walks)
        lab = np.zeros(len(walks), np.int32)
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*no cluster table'):
            c.cluster_path_containment()
        c.cluster_table(lab)
        c.cluster_loci()
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_paths first'):
            c.cluster_path_containment()
        assert get_rows(c, 0, 0, 0, 0)[0] == _lib.FSLR_ERR_STATE              # a failed call installed nothing
        with pytest.raises(_lib.FslrError, match=STATE):
            c.cluster_path_containment_timings()
        want_p = pr.paths_of_csr(idx.csr, lab, key, rev)
        want = cr.containment(want_p)
        nr, npairs = len(want_p['n_reads']), len(want['outer'])
        assert nr == 5 and npairs >= 4
        got_p, got = device(c, key, rev, loci=False)
        same(got, want)
        assert c.cluster_path_containment_timings()['containment'] > 0
        # two runs give the same bytes; the getter answers for the resident rows
        again = dict(zip(cr.NAMES, c.cluster_path_containment()))
        assert [again[k].tobytes() for k in cr.NAMES] == [want[k].tobytes() for k in cr.NAMES]
        rc, res = get_rows(c, nr, npairs, nr, npairs)
        assert rc == _lib.FSLR_OK
        same(res, want)
        # a small capacity is refused and nothing is written
        for caps in ((nr - 1, npairs), (nr, npairs - 1)):
            rc, res = get_rows(c, nr, npairs, *caps)
            assert rc == _lib.FSLR_ERR_INVALID and b'capacity' in c._L.fslr_last_error(c._h)
            assert all((res[k] == (249 if k == 'rev' else -7)).all() for k in cr.NAMES)
        # NULL outputs are skipped
        n_occ = np.full(npairs, -7, np.int32)
        assert c._L.fslr_get_cluster_path_containment(c._h, None, None, None, None, _lib._ptr(n_occ), None, None, None, None,
                                                      nr, npairs) == _lib.FSLR_OK
        np.testing.assert_array_equal(n_occ, want['n_occ'])
        # the path, loci and junction rows are left alone
        path_rows_equal(c, want_p)
        # new path rows, new loci rows and a new table each drop the rows
        c.cluster_paths_any(key, rev)
        assert get_rows(c, nr, npairs, nr, npairs)[0] == _lib.FSLR_ERR_STATE
        same(dict(zip(cr.NAMES, c.cluster_path_containment())), want)
        c.cluster_loci()
        assert get_rows(c, nr, npairs, nr, npairs)[0] == _lib.FSLR_ERR_STATE
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_paths first'):
            c.cluster_path_containment()
        same(device(c, key, rev, loci=False)[1], want)
        c.cluster_table(lab)
        assert get_rows(c, nr, npairs, nr, npairs)[0] == _lib.FSLR_ERR_STATE
        same(device(c, key, rev)[1], want)
    finally:
        c.close()


def test_append_and_remove_leave_a_stale_table_whose_rows_still_answer():
    data, qstart, rev, cid_of_code = cs.truncated_fixture('cfg1_1k_x3')
    codes = np.unique(data.qcode)
    late = np.isin(data.qcode, codes[codes.size * 2 // 3:])
    idx = cluster.build_interval_trees(data.select(~late))
    try:
        c = idx.ctx
        first = idx.cluster_path_containment(qstart[~late], rev[~late], cs.labels_for(idx.csr, cid_of_code))
        want = {k: getattr(first, k) for k in cr.NAMES}
        same(want, cr.containment({k: getattr(first.paths, k) for k in pr.NAMES}))
        assert len(first) > 50 and 0 < int(first.rev.sum()) < len(first)           # contained pairs, both directions
        idx.append(data.select(late))
        # the table is stale for the calls that read the reads; the path rows it describes and their containment stand
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_table again'):
            c.cluster_paths(np.zeros(idx.csr.n_intervals, np.int32))
        rc, res = get_rows(c, len(first.paths), len(first), len(first.paths), len(first))
        assert rc == _lib.FSLR_OK
        same(res, want)
        same(dict(zip(cr.NAMES, c.cluster_path_containment())), want)
        keep = np.ones(idx.csr.n_reads, bool)
        keep[0] = False
        idx.remove(keep=keep)
        same(dict(zip(cr.NAMES, c.cluster_path_containment())), want)
    finally:
        idx.ctx.close()


def test_multi_gpu_index_refuses():
    mg = cluster.MultiGpuIndex(sr.make_data([1, 1], [0, 5], [9, 9]), 2)
    with pytest.raises(NotImplementedError, match='n_gpus=1'):
        mg.cluster_path_containment([0, 1])


# ------------------------------------------------------------------ 9. the command line
def expected_text(p, want):
    """The file of --cluster-path-containment for the path rows ``p`` and their containment ``want``, from the plain
    statement alone."""
    of_row = np.repeat(np.arange(len(p['off']) - 1), np.diff(p['off'])).tolist()
    lens, co = np.diff(p['tok_off']).tolist(), want['coff'].tolist()
    lines = ['cluster\trow\tn_tokens\tn_reads\tn_inner\tsupport\tmaximal\tcollapse_to\tcollapsed_reads\tcontained_in']
    for r in range(len(lens)):
        entries = [f"{want['outer'][k]}:{want['offset'][k]}:{'-' if want['rev'][k] else '+'}" for k in range(co[r], co[r + 1])]
        lines.append('\t'.join(map(str, (of_row[r], r, lens[r], p['n_reads'][r], want['n_inner'][r], want['support'][r],
                                         int(co[r] == co[r + 1]), want['collapse_to'][r], want['collapsed_reads'][r],
                                         ','.join(entries) or '.'))))
    return '\n'.join(lines) + '\n'


def test_the_writer_on_truncated_reads_lists_the_outers_of_both_directions(tmp_path):
    """main.write_cluster_path_containment, the function behind the flag, on the fixture with truncated reads: it
    reads qstart and the strands from the fixture's .mappings.bed by the data list's row numbers, and the last
    column holds outer:offset:strand entries of both directions."""
    from fslr_amd.main import write_cluster_path_containment
    name = 'cfg1_1k_x3'
    data, qstart, rev, cid_of_code = cs.truncated_fixture(name)
    bed = os.path.join(str(tmp_path), 'fx.mappings.bed')
    with open(bed, 'w') as fh:
        fh.write(fx.input_bed_text(name))
    out = os.path.join(str(tmp_path), 'out.bed')
    idx = cluster.build_interval_trees(data)
    try:
        csr = idx.csr
        pos = np.asarray(csr.data_pos, np.int64)
        lab = cs.labels_for(csr, cid_of_code)
        assert write_cluster_path_containment(out, bed, idx, lab)
    finally:
        idx.ctx.close()
    p = pr.paths_of_csr(csr, lab, qstart[pos], rev[pos])
    want = cr.containment(p)
    assert len(want['outer']) > 100 and 0 < int(want['rev'].sum()) < len(want['outer'])
    text = open(out).read()
    assert text == expected_text(p, want)
    last = [ln.split('\t')[-1] for ln in text.splitlines()[1:]]
    assert sum(e.endswith(':-') for e in last) > 10 and sum(e.endswith(':+') for e in last) > 10 and '.' in last


@pytest.mark.parametrize('io_flag', ['--native-io', '--pandas-io'])
def test_cli_cluster_path_containment_in_both_io_modes(tmp_path, io_flag):
    """The flag end to end in both I/O modes.  The fixture's own clusters hold no contained path (every row is
    maximal and the last column is '.' throughout): what this covers is the flag's plumbing and the per-row columns;
    the entries of the last column are the writer test's above and tests/test_containment_binding.py's."""
    name = 'cfg1_1k_x3'
    data, csr, cid, nc, kw = fixture_membership(name)
    qstart, _, rev = bed_inputs(name, data)
    pos = np.asarray(csr.data_pos, np.int64)
    p = pr.paths(csr.read_off, csr.iv_chrom, csr.iv_start, csr.iv_end, cid, nc, qstart[pos], rev[pos])
    want = cr.containment(p)
    res = run_cli(name, str(tmp_path), io_flag, '--cluster-path-containment')
    assert res.exit_code == 0, (res.output, res.exception)
    text = open(os.path.join(str(tmp_path), 'fx.mappings.cluster_path_containment.bed')).read()
    assert text == expected_text(p, want)
    assert text.count('\n') > 10
    for which in ('cluster', 'representative'):
        assert open(os.path.join(str(tmp_path), f'fx.mappings.{which}.bed')).read() == fx.expected_text(name, which), which


def test_cli_refuses_several_gpus(tmp_path):
    res = run_cli('cfg1_1k_x3', str(tmp_path), '--cluster-path-containment', '--gpus=2')
    assert res.exit_code == 2 and '--gpus 1' in res.output
    assert sorted(os.listdir(str(tmp_path))) == ['fx.bwa_dodi.bam', 'fx.mappings.bed']
