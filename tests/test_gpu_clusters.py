"""The cluster table and the representatives on the device (fslr_cluster_table, fslr_get_cluster_ids,
fslr_get_cluster_members, fslr_assign_clusters, fslr_choose_representatives) against tests/cluster_ref.py,
which tests/test_cluster_table_host.py pins to the reference's own outputs.  Every comparison is exact."""
import numpy as np
import pandas as pd
import pytest

import cluster_ref as cr
import fixtures as fx
from fslr_amd import _lib, cluster, ingest, main

pytestmark = pytest.mark.gpu

INVALID = f'fslr error {_lib.FSLR_ERR_INVALID}'
STATE = f'fslr error {_lib.FSLR_ERR_STATE}'


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def device_table(ctx, labels):
    info = ctx.cluster_table(labels)
    cid, size = ctx.cluster_ids()
    off, members = ctx.cluster_members()
    return {'cid': cid, 'size': size, 'off': off, 'members': members, 'roots': members[off[:-1]], **info}


def same_table(got, want):
    for k in ('n_clusters', 'n_nodes', 'max_size'):
        assert got[k] == want[k], k
    for k in ('cid', 'size', 'off', 'members', 'roots'):
        assert got[k].dtype == want[k].dtype, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def check(ctx, labels):
    labels = np.asarray(labels, np.int32)
    assert cr.valid_labels(labels) == -1
    want = cr.table(labels)
    same_table(device_table(ctx, labels), want)
    return want


def labels_of(n, comps):
    lab = np.arange(n, dtype=np.int32)
    for c in comps:
        c = np.asarray(c)
        lab[c] = c.min()
    return lab


# ------------------------------------------------------------------ 1. golden fixtures
@pytest.mark.parametrize('name', cr.golden_fixtures())
def test_golden_fixtures(ctx, name):
    case = cr.fixture_case(name)
    t = check(ctx, case['labels'])
    assert t['n_clusters'] == len(case['components'])
    present = np.ones(case['n_codes'], bool)
    cl, nr, k = ctx.assign_clusters(present, case['code_of_rank'])
    avg, win = ctx.choose_representatives(cl, case['score_sum'], case['score_cnt'], case['first_row'],
                                          t['n_clusters'] + k)
    cr.check_fixture_outputs(case, cl, nr, k, avg, win)
    assert (k == 0) == (name == 'longcap_240')           # the one fixture with int columns (no read alone)


def test_noclusters_fixture(ctx):
    from host_pipeline import host_prepare
    assert fx.stage('noclusters')['components'] == []
    n = host_prepare('noclusters')[0].csr().n_reads
    t = check(ctx, np.arange(n))
    assert t['n_clusters'] == 0 and t['n_nodes'] == 0 and t['max_size'] == 0
    cl, nr, k = ctx.assign_clusters(np.ones(n, bool))
    assert k == n and cl.tolist() == list(range(n)) and (nr == 1).all()


# ------------------------------------------------------------------ 2. boundary shapes
@pytest.mark.parametrize('n', [0, 1, 2])
def test_tiny(ctx, n):
    check(ctx, np.arange(n))
    check(ctx, np.zeros(n, np.int32))
    if n == 0:
        off, members = ctx.cluster_members()
        assert off.tolist() == [0] and members.size == 0


def test_all_singletons_and_one_component(ctx):
    n = 70_001
    t = check(ctx, np.arange(n))
    assert t['n_clusters'] == 0
    t = check(ctx, np.zeros(n, np.int32))
    assert (t['n_clusters'], t['n_nodes'], t['max_size']) == (1, n, n)


SIZES = (63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
# hipcub's scans and sorts tile the input by 256 threads x a few items: 1024 .. 4096 and 3840 = 256 x 15
EDGES = (64, 256, 1024, 2048, 3840, 4096)


def test_component_sizes_at_wave_and_block_edges(ctx):
    rng = np.random.default_rng(7)
    n = 3 * sum(SIZES)
    for scattered in (False, True):
        ranks = rng.permutation(n) if scattered else np.arange(n)
        comps, at = [], 0
        for s in SIZES:
            comps.append(ranks[at:at + s])
            at += s + int(rng.integers(0, 3))           # a few reads alone in between
        t = check(ctx, labels_of(n, comps))
        assert sorted(np.diff(t['off']).tolist()) == sorted(SIZES)


def test_roots_on_and_beside_tile_edges(ctx):
    n = 3 * 4096 + 600
    roots = sorted({p * m + d for p in EDGES for m in (1, 2, 3) for d in (-1, 0, 1) if p * m + d < 3 * 4096})
    spare = np.setdiff1d(np.arange(n), roots)[::-1]    # each root's only member: a high rank
    comps = [[r, int(spare[k])] for k, r in enumerate(roots)]
    t = check(ctx, labels_of(n, comps))
    assert t['roots'].tolist() == roots
    # every other read alone, then every read from an edge on in one component
    for p in (64, 256, 3840):
        check(ctx, np.where(np.arange(n) >= p, p, np.arange(n)))


def test_alternating_components_keep_rank_order(ctx):
    n = 5000
    a, b = np.arange(100, 4100, 2), np.arange(101, 4101, 2)
    t = check(ctx, labels_of(n, [a, b]))
    assert t['members'][:a.size].tolist() == a.tolist() and t['members'][a.size:].tolist() == b.tolist()


def test_root_at_the_end(ctx):
    for n in (2, 65, 4097):
        t = check(ctx, labels_of(n, [[n - 2, n - 1]]))
        assert t['roots'].tolist() == [n - 2] and t['cid'][-2:].tolist() == [0, 0]


# ------------------------------------------------------------------ 3. contention and determinism
def test_one_large_component_and_determinism(ctx):
    rng = np.random.default_rng(11)
    n = 300_000
    perm = rng.permutation(n)
    comps = [perm[:100_000]]
    at = 100_000
    for s in rng.integers(2, 9, 4000).tolist():
        comps.append(perm[at:at + s])
        at += s
    lab = labels_of(n, comps)
    want = check(ctx, lab)
    assert want['max_size'] == 100_000 and want['n_clusters'] == 4001
    code_of_rank = rng.permutation(n).astype(np.int64)
    present = rng.random(n) < 0.9
    sums, cnt = rng.integers(-10**6, 10**6, n), rng.integers(0, 5, n)
    first_row = rng.permutation(n).astype(np.int64)
    runs = []
    for _ in range(2):
        t = device_table(ctx, lab)
        cl, nr, k = ctx.assign_clusters(present, code_of_rank)
        avg, win = ctx.choose_representatives(cl, sums, cnt, first_row, want['n_clusters'] + k)
        runs.append([t[x].tobytes() for x in ('cid', 'size', 'off', 'members')] +
                    [cl.tobytes(), nr.tobytes(), avg.tobytes(), win.tobytes()])
    assert runs[0] == runs[1]
    wcl, wnr, wk = cr.assign(want, present, code_of_rank)
    np.testing.assert_array_equal(cl, wcl)
    np.testing.assert_array_equal(nr, wnr)
    assert k == wk
    wavg, wwin = cr.choose(wcl, sums, cnt, first_row, want['n_clusters'] + wk)
    assert avg.view(np.int64).tolist() == wavg.view(np.int64).tolist()
    np.testing.assert_array_equal(win, wwin)


# ------------------------------------------------------------------ 4. random forests
@pytest.mark.parametrize('seed', [1, 2, 3])
def test_random_forests(ctx, seed):
    rng = np.random.default_rng(seed)
    n = 200_000
    is_root = rng.random(n) < (0.1, 0.4, 0.8)[seed - 1]
    is_root[0] = True
    roots = np.flatnonzero(is_root)
    before = np.cumsum(is_root)                          # roots at or below each rank
    lab = roots[(rng.random(n) * before).astype(np.int64)]
    lab[roots] = roots
    check(ctx, lab)


# ------------------------------------------------------------------ 5. invalid host labels
def test_invalid_labels_leave_the_table(ctx):
    good = labels_of(1000, [[3, 7, 900], [10, 11]])
    before = device_table(ctx, good)
    above = good.copy()
    above[500] = 501
    negative = good.copy()
    negative[640] = -1
    chained = good.copy()
    chained[700], chained[800] = 7, 11                  # labels[7] = 3 and labels[11] = 10: both not roots
    for lab, r in ((above, 500), (negative, 640), (chained, 700)):
        assert cr.valid_labels(lab) == r
        with pytest.raises(_lib.FslrError, match=rf'{INVALID}.*labels\[{r}\] = {lab[r]}\b'):
            ctx.cluster_table(lab)
        cid, size = ctx.cluster_ids()
        off, members = ctx.cluster_members()
        np.testing.assert_array_equal(cid, before['cid'])
        np.testing.assert_array_equal(size, before['size'])
        np.testing.assert_array_equal(off, before['off'])
        np.testing.assert_array_equal(members, before['members'])


# ------------------------------------------------------------------ 6. state handling
def test_state_errors():
    c = _lib.Context(0)
    try:
        with pytest.raises(_lib.FslrError, match=STATE):
            c.cluster_ids()
        with pytest.raises(_lib.FslrError, match=STATE):
            c.cluster_members()
        with pytest.raises(_lib.FslrError, match=STATE):
            c.assign_clusters(np.ones(3, bool))
        with pytest.raises(_lib.FslrError, match=STATE):
            c.cluster_table()
        with pytest.raises(_lib.FslrError, match=STATE):
            c.cluster_timings()
    finally:
        c.close()


def test_virtual_reads_are_refused():
    import search_ref as sr
    rng = np.random.default_rng(44)
    n = 400
    qcode = np.concatenate([np.zeros(70, np.int64), 1 + rng.integers(0, 100, n - 70)])
    start = rng.integers(0, 200, n) * 500
    data = sr.make_data(rng.integers(1, 3, n), start, start + rng.integers(50, 2500, n), qcode=qcode)
    idx = cluster.build_interval_trees(data)
    try:
        assert idx.long is not None
        with pytest.raises(_lib.FslrError, match=f'{INVALID}.*virtual'):
            idx.ctx.cluster_table()
        check(idx.ctx, labels_of(50, [[1, 2]]))         # host labels are taken
    finally:
        idx.ctx.close()


# ------------------------------------------------------------------ 7. the context's own labels
def test_device_labels_path():
    from host_pipeline import host_prepare
    name = 'mixed_2k_l8'
    case = cr.fixture_case(name)
    data, _, kw = host_prepare(name)
    idx = cluster.build_interval_trees(data)
    c = idx.ctx
    try:
        g = cluster.query_graph(idx, data, kw['overlap'], [float(x) for x in kw['jaccard_cutoffs'].split(',')], 10,
                                kw['qlen_diff'], kw['n_alignment_diff'])
        labels = c.labels()
        np.testing.assert_array_equal(labels, case['labels'])
        ne = g.n_edges
        edges = [x.copy() for x in c.edges(ne)]
        dense = idx._dense_chroms(data.chrom[:50])
        soff, shits = c.search(dense, idx._coords(data.start[:50]), idx._coords(data.end[:50]))
        total = c._search(dense, idx._coords(data.start[:50]), idx._coords(data.end[:50]), None)   # the saved batch
        c.coverage_build([0, 0, 1], [5, 10, 7], [50, 20, 9], 2)
        depth = c.coverage_at([0, 0, 1], [12, 30, 8])
        info = c.cluster_table()
        assert info['n'] == labels.size
        cid, size = c.cluster_ids()
        off, members = c.cluster_members()
        want = cr.table(case['labels'])
        same_table({'cid': cid, 'size': size, 'off': off, 'members': members, 'roots': members[off[:-1]], **info}, want)
        same_table(device_table(c, labels), want)
        c.cluster_table()                                # back on the device labels
        cl, nr, k = c.assign_clusters(np.ones(case['n_codes'], bool), case['code_of_rank'])
        avg, win = c.choose_representatives(cl, case['score_sum'], case['score_cnt'], case['first_row'],
                                            want['n_clusters'] + k)
        cr.check_fixture_outputs(case, cl, nr, k, avg, win)
        # the query state, the saved search batch and the coverage set are as they were
        np.testing.assert_array_equal(c.labels(), labels)
        for a, b in zip(c.edges(ne), edges):
            np.testing.assert_array_equal(a, b)
        hits = np.empty(total, np.int32)
        c._check(c._L.fslr_search_hits(c._h, _lib._ptr(hits), total))
        np.testing.assert_array_equal(hits, shits)
        np.testing.assert_array_equal(c.coverage_at([0, 0, 1], [12, 30, 8]), depth)
    finally:
        c.close()


# ------------------------------------------------------------------ 8. assign
def test_assign_codes(ctx):
    rng = np.random.default_rng(3)
    n, nc = 5000, 6000
    lab = labels_of(n, [rng.permutation(n)[:700], [4000, 4001], [10, 4999]])
    t = check(ctx, lab)
    code_of_rank = rng.permutation(nc)[:n].astype(np.int64)      # 1000 codes no rank names
    present = rng.random(nc) < 0.8
    cl, nr, k = ctx.assign_clusters(present, code_of_rank)
    wcl, wnr, wk = cr.assign(t, present, code_of_rank)
    np.testing.assert_array_equal(cl, wcl)
    np.testing.assert_array_equal(nr, wnr)
    assert k == wk and cl.dtype == np.int64 and nr.dtype == np.int64
    unnamed = np.setdiff1d(np.arange(nc), code_of_rank)
    single = np.flatnonzero(present & (wcl >= t['n_clusters']))
    assert np.intersect1d(unnamed[present[unnamed]], single).size == present[unnamed].sum() > 0
    assert np.all(np.diff(cl[single]) == 1) and cl[single[0]] == t['n_clusters']     # ascending code order
    assert (cl[~present] == -1).all() and (nr[~present] == 0).all()
    # the identity
    cl, nr, k = ctx.assign_clusters(np.ones(n, bool))
    wcl, wnr, wk = cr.assign(t, np.ones(n, bool))
    np.testing.assert_array_equal(cl, wcl)
    np.testing.assert_array_equal(nr, wnr)
    with pytest.raises(_lib.FslrError, match=INVALID):
        ctx.assign_clusters(np.ones(n + 1, bool))                # the identity needs n_codes == n
    dup = code_of_rank.copy()
    dup[3000] = dup[20]
    dup[4000] = dup[30]
    with pytest.raises(_lib.FslrError, match=f'{INVALID}.*rank 3000 names code {dup[20]}\\b'):
        ctx.assign_clusters(present, dup)
    out = code_of_rank.copy()
    out[1234] = nc
    out[77] = -1
    with pytest.raises(_lib.FslrError, match=f'{INVALID}.*rank 77 names code -1\\b'):
        ctx.assign_clusters(present, out)


def _frame_and_graph(name):
    """The CLI's pandas frame (the reader's qname codes attached, as ingest.frame_from does) and a
    ClusterGraph with the reference's components."""
    case = cr.fixture_case(name)
    bed = fx.input_bed(name)
    codes, uniq = pd.factorize(bed['qname'])
    qc = ingest.QnameCodes(codes.astype(np.int64), np.asarray(uniq, dtype=object))
    bed.attrs[ingest.ATTR] = qc
    if fx.cli_options(name)['filter_false']:
        bed = cluster.delete_false(bed)
        bed.attrs[ingest.ATTR] = qc
    n = case['labels'].size
    G = cluster.ClusterGraph(case['names'], case['labels'], (np.zeros(0, np.int32), np.zeros(0, np.int32)),
                             np.zeros(n, np.int32), {})
    return case, bed, G


@pytest.mark.parametrize('name', ['longcap_240', 'capbind_1500', 'edge_cases', 'edge_cases_ff'])
def test_assign_clusters_frame(ctx, name):
    case, bed, G = _frame_and_graph(name)
    host = main.assign_clusters(bed.copy(), G)
    dev = main.assign_clusters(bed.copy(), G, ctx=ctx)
    kind = 'i' if name == 'longcap_240' else 'f'       # k == 0 gives int columns, k > 0 float ones
    for col in ('cluster', 'n_reads'):
        assert dev[col].dtype == host[col].dtype and dev[col].dtype.kind == kind
        np.testing.assert_array_equal(dev[col].to_numpy(), host[col].to_numpy())
        np.testing.assert_array_equal(dev[col].to_numpy(), case['cluster_bed'][col].to_numpy())


# ------------------------------------------------------------------ 9. representatives
def test_representative_ties(ctx):
    # exact (sum, cnt) pairs whose quotients are 0.75 and the next double above it (sums below 2**53)
    lo, hi = (3 * 2**51, 2**53), (3 * 2**51 + 1, 2**53)
    assert lo[0] / lo[1] == 0.75 and hi[0] / hi[1] == np.nextafter(0.75, 1.0)
    rows = [  # cluster, sum, cnt, first_row
        (0, 2, 1, 50), (0, 4, 2, 20), (0, 6, 3, 30),            # equal means from different rationals: row 20
        (1, -9, 3, 5), (1, -4, 2, 9), (1, -30, 10, 1),          # negative sums: -2 beats -3
        (2, lo[0], lo[1], 1), (2, hi[0], hi[1], 2),             # one ulp apart: the larger, whatever the rows
        (3, 17, 4, 8),                                          # alone
        (-1, 5, 1, 0), (4, 5, 0, 0),                            # skipped: no cluster, no rows
        (6, 0, 3, 4), (6, 0, 1, 3), (6, -1, 7, 2),              # zero means tie: row 3
    ]
    cl, s, q, fr = (np.asarray(x, np.int64) for x in zip(*rows))
    avg, win = ctx.choose_representatives(cl, s, q, fr, 8)
    assert win.tolist() == [1, 4, 7, 8, -1, -1, 12, -1]
    assert np.isnan(avg[[9, 10]]).all() and not np.isnan(np.delete(avg, [9, 10])).any()
    wavg, wwin = cr.choose(cl, s, q, fr, 8)
    assert avg.view(np.int64).tolist() == wavg.view(np.int64).tolist() and win.tolist() == wwin.tolist()


def test_representative_means_bit_for_bit(ctx):
    rng = np.random.default_rng(9)
    n, n_out = 100_000, 30_000
    s = rng.integers(-(1 << 52), 1 << 52, n)
    s[:20_000] = rng.integers(-5000, 5000, 20_000)
    q = rng.integers(1, 60, n)
    cl = rng.integers(0, n_out, n)
    cl[rng.random(n) < 0.05] = -1
    cl[:3000] = 7                                        # one crowded cluster with many tied means
    s[:3000], q[:3000] = rng.integers(0, 3, 3000) * q[:3000], q[:3000]
    fr = rng.permutation(n).astype(np.int64)
    avg, win = ctx.choose_representatives(cl, s, q, fr, n_out)
    want = s.astype(np.float64) / q.astype(np.float64)
    keep = cl >= 0
    assert avg[keep].view(np.int64).tolist() == want[keep].view(np.int64).tolist()
    assert np.isnan(avg[~keep]).all()
    wavg, wwin = cr.choose(cl, s, q, fr, n_out)
    np.testing.assert_array_equal(win, wwin)


def test_representative_errors(ctx):
    one = np.ones(4, np.int64)
    big = one.copy()
    big[2], big[3] = 1 << 53, -(1 << 53)
    with pytest.raises(_lib.FslrError, match=f'{INVALID}.*code 2 '):
        ctx.choose_representatives(one * 0, big, one, np.arange(4), 1)
    ok = one.copy()
    ok[2] = (1 << 53) - 1
    avg, win = ctx.choose_representatives(one * 0, ok, one, np.arange(4), 1)
    assert win.tolist() == [2] and avg[2] == float((1 << 53) - 1)
    with pytest.raises(_lib.FslrError, match=f'{INVALID}.*code 1 .*n_out = 3'):
        ctx.choose_representatives(np.asarray([0, 3, 2, 5]), one, one, np.arange(4), 3)
    with pytest.raises(_lib.FslrError, match=f'{INVALID}.*code 3 '):
        ctx.choose_representatives(one * 0, one, np.asarray([1, 0, 2, -1]), np.arange(4), 1)
    avg, win = ctx.choose_representatives(np.zeros(0, np.int64), [], [], [], 2)
    assert avg.size == 0 and win.tolist() == [-1, -1]


@pytest.mark.parametrize('name', ['mixed_2k_l8', 'ties_600', 'edge_cases'])
def test_choose_alignment_frame(ctx, name):
    case, bed, G = _frame_and_graph(name)
    frame = main.assign_clusters(bed, G)
    assert cluster._choose_alignment_codes(frame.copy()) is not None      # the frame the device path takes
    host = cluster.choose_alignment(frame.copy())
    dev = cluster.choose_alignment(frame.copy(), ctx=ctx)
    assert dev.index.tolist() == host.index.tolist()
    assert dev['avg_alignment_score'].to_numpy().view(np.int64).tolist() == \
        host['avg_alignment_score'].to_numpy().view(np.int64).tolist()
    assert dev['qname'].tolist() == case['representative_bed']['qname'].tolist()


# ------------------------------------------------------------------ 10. get_subgraphs
@pytest.mark.parametrize('name', ['mixed_2k_l8', 'capbind_1500'])
def test_get_subgraphs_on_the_device(ctx, name):
    case, _, G = _frame_and_graph(name)
    host = cluster.get_subgraphs(G)
    dev = cluster.get_subgraphs(G, ctx=ctx)
    assert dev == host == [set(c) for c in case['components']]
    t = cluster.cluster_table(G, ctx=ctx)
    assert isinstance(t, cluster.ClusterTable) and len(t) == len(host)
    np.testing.assert_array_equal(t.roots, G.roots)
    np.testing.assert_array_equal(t.cid, G.component_id)
    np.testing.assert_array_equal(t.size, G.comp_size)


def test_timings():
    c = _lib.Context(0, profiling=True)
    try:
        c.cluster_table(labels_of(10_000, [[1, 5, 9000], [2, 3]]))
        c.assign_clusters(np.ones(10_000, bool))
        c.choose_representatives(np.zeros(10, np.int64), np.arange(10), np.ones(10, np.int64), np.arange(10), 1)
        tm = c.cluster_timings()
        assert set(tm) == {'table', 'assign', 'choose'} and all(v > 0 for v in tm.values())
    finally:
        c.close()
