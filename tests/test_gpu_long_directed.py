"""Directed GPU tests for reads of more than FSLR_MAX_L (64) intervals: chunk seams, the 4096
limit, dense blocks, first-fit conflicts across a seam, every rank order, buffer growth and context reuse.

The inputs and the expected graphs come from tests/long_ref.py, a plain restatement of the reference's pair
loop that tests/test_long_ref.py holds against the C oracle without a GPU.  Every comparison is exact: edges
(a, b, I, U), forward degrees, labels and components.  Two device paths decide pairs with a long read: the
sweep's match entries split, sorted and matched per pair (long.hip, engine 'sweep+long', overlap > 0), and the
wave-wide general evaluator (firstfit.hpp long_fit in cap.hip's k_cap_eval, engine 'pairs', overlap <= 0:
every same-chromosome cell matches there, so the full-block and diagonal inputs become dense).
"""
import dataclasses

import numpy as np
import pytest

import long_ref as R
from fslr_amd import _lib, cluster
from fslr_amd.prep import fold_overlap_threshold, pass_table, umax_table

pytestmark = pytest.mark.gpu

QCUT, NCUT = 1 - R.QLEN_DIFF, 1 - R.NAL_DIFF
ERR_STATE = f'fslr error {_lib.FSLR_ERR_STATE}'


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _sorted_edges(a, b, I, U):
    return sorted(zip(a.tolist(), b.tolist(), I.tolist(), U.tolist()))


def _n_long_edges(csr, edges):
    L = np.diff(csr.read_off)
    return sum(1 for e in edges if L[e[0]] > _lib.FSLR_MAX_L or L[e[1]] > _lib.FSLR_MAX_L)


def _query_equals(idx, data, overlap, cuts, want, engine):
    """cluster.query_graph (what query_interval_trees wraps: the same edges with I and U as integers) and the
    ClusterGraph of its result against the reference's graph."""
    g = cluster.query_graph(idx, data, overlap, cuts, 10, R.QLEN_DIFF, R.NAL_DIFF)
    assert g.stats['engine'] == engine
    assert _sorted_edges(g.a, g.b, g.I, g.U) == want.edges
    G = cluster.ClusterGraph(data.qnames[g.csr.read_qcode], g.labels, (g.a, g.b), g.fwd, g.stats)
    np.testing.assert_array_equal(G.fwd, want.fwd)
    np.testing.assert_array_equal(G.labels, want.labels)
    np.testing.assert_array_equal(G.component_id, want.comp)
    assert G.stats['max_fwd'] == want.fwd.max()
    assert G.stats['long_pair_edges'] == (len(want.edges) if engine == 'pairs' else _n_long_edges(g.csr, want.edges))
    return g


@pytest.mark.parametrize('case', R.CASES, ids=repr)
def test_directed_input_vs_reference(ctx, case):
    """Each input at its positive overlap with both of its cutoff lists (the sweep, k_long_split, the sort and
    k_long_greedy) and at overlap 0.0 and -0.5 with [0.3] (k_cap_eval's long_fit over the whole lists)."""
    data = case.data()
    idx = cluster.build_interval_trees(data, ctx=ctx)
    assert idx.long is not None and int(idx.long.max()) == case.max_len
    for cuts in case.cuts:
        _query_equals(idx, data, case.overlap, cuts, case.ref(case.overlap, cuts), 'sweep+long')
    for overlap in (0.0, -0.5):
        _query_equals(idx, data, overlap, [0.3], case.ref(overlap, [0.3]), 'pairs')


@pytest.mark.parametrize('name', ['diag_65_64', 'block_130_64_130', 'g63_64x0_127_swapped'])
def test_query_interval_trees_outputs(ctx, name):
    """The public call: match_df's rows are the reference's edges with I / U as a Python float."""
    case = R.CASE[name]
    data = case.data()
    idx = cluster.build_interval_trees(data, ctx=ctx)
    match_df, G = cluster.query_interval_trees(idx, data, case.overlap, case.cuts[0], 10, R.QLEN_DIFF, R.NAL_DIFF)
    want = case.ref(case.overlap, case.cuts[0])
    names = data.qnames[data.csr().read_qcode]
    assert list(zip(match_df['query1'], match_df['query2'], match_df['jaccard_similarity'])) == \
        [(names[a], names[b], i / u) for a, b, i, u in want.edges]
    assert sorted(zip(*[x.tolist() for x in G.edges_ab])) == [e[:2] for e in want.edges]
    np.testing.assert_array_equal(G.fwd, want.fwd)
    np.testing.assert_array_equal(G.component_id, want.comp)
    assert G.stats['engine'] == 'sweep+long'


# ---------------------------------------------------------------------------------- the C ABI
def _abi_query(ctx, csr, overlap, cuts):
    """fslr_set_reads_any .. fslr_long_query through the binding, as cluster._query_long drives them: the long
    edge list, the context's own (short-short) edges, forward degrees over both and the labels."""
    n = csr.n_reads
    ctx.load_csr_any(csr, np.zeros(csr.n_intervals, np.int32))
    ctx.build_index()
    ctx.set_thresholds(fold_overlap_threshold(csr.iv_aln, overlap))
    ctx.set_long_cutoffs(umax_table(cuts, int(np.diff(csr.read_off).max())))
    ctx.reserve_edges(1 << 16)
    n_long = ctx.long_query(QCUT, NCUT, pass_table(cuts), 10)
    st = ctx.stats()
    la, lb, lI, lU = ctx.long_edges(n_long)
    sa, sb, sI, sU = ctx.edges(st['n_edges'])
    ctx.components()
    if n_long:
        ctx.union_pairs(la, lb, n_long, on_device=False)
        ctx.finalize_labels()
    return _sorted_edges(la, lb, lI, lU), _sorted_edges(sa, sb, sI, sU), ctx.labels()[:n]


def _abi_equals(ctx, data, overlap, cuts):
    csr = data.csr()
    want = R.long_ref(csr, overlap, cuts)
    L = np.diff(csr.read_off)
    is_long = lambda e: L[e[0]] > _lib.FSLR_MAX_L or L[e[1]] > _lib.FSLR_MAX_L
    long_e, short_e, labels = _abi_query(ctx, csr, overlap, cuts)
    assert long_e == [e for e in want.edges if is_long(e)]          # I and U as they are, beyond a byte
    assert short_e == [e for e in want.edges if not is_long(e)]
    np.testing.assert_array_equal(labels, want.labels)
    return long_e, short_e, labels.tolist()


@pytest.mark.parametrize('name', ['diag_4096_4096', 'diag_4095_4096', 'last_tail', 'last_row0', 'last_col0',
                                  'block_130_130_64', 'block_64_130_130', 'block_257_129', 'g127_128x64_128',
                                  'g63_64x38_39_short_swapped', 'gate_equal', 'many_chromosomes'])
def test_abi_long_and_short_edge_lists(ctx, name):
    """fslr_get_long_edges holds exactly the pairs with a long read (I and U unclamped: up to 4096 and 8191),
    fslr_get_edges exactly the pairs of two short reads."""
    case = R.CASE[name]
    cuts = case.cuts[1] if name.startswith('block') else case.cuts[0]      # [0.3]: 64 / 130 is an edge too
    long_e, short_e, _ = _abi_equals(ctx, case.data(), case.overlap, cuts)
    assert long_e and short_e
    if case.pair is not None:
        assert case.pair in [e[2:] for e in long_e]


# ---------------------------------------------------------------------------------- limits
def test_read_of_4097_intervals_is_refused_then_the_context_works(ctx):
    too_long = R.diagonal(R.MAX_READ + 1, 65)
    assert int(np.diff(too_long.csr().read_off).max()) == R.MAX_READ + 1
    with pytest.raises(_lib.FslrError, match=r'every read needs 1\.\.4096 intervals'):
        cluster.build_interval_trees(too_long, ctx=ctx)
    with pytest.raises(_lib.FslrError, match=r'every read needs 1\.\.4096 intervals'):
        ctx.load_csr_any(too_long.csr(), np.zeros(len(too_long), np.int32))
    case = R.CASE['diag_4096_4096']
    idx = cluster.build_interval_trees(case.data(), ctx=ctx)
    _query_equals(idx, case.data(), 0.8, [0.5], case.ref(0.8, [0.5]), 'sweep+long')
    _query_equals(idx, case.data(), 0.0, [0.3], case.ref(0.0, [0.3]), 'pairs')


def test_read_of_no_intervals_is_refused(ctx):
    csr = R.CASE['diag_65_65'].data().csr()
    off = np.concatenate([csr.read_off[:2], csr.read_off[1:]])              # read 1 of 0 intervals
    grown = lambda x: np.concatenate([x[:1], x])
    empty = dataclasses.replace(csr, read_off=off, read_qlen2=grown(csr.read_qlen2), read_nal=grown(csr.read_nal),
                                read_qcode=grown(csr.read_qcode))
    assert np.diff(empty.read_off).min() == 0 and np.diff(empty.read_off).max() == 65
    with pytest.raises(_lib.FslrError, match=r'every read needs 1\.\.4096 intervals'):
        ctx.load_csr_any(empty, np.zeros(empty.n_intervals, np.int32))
    _abi_equals(ctx, R.CASE['diag_65_65'].data(), 0.8, [0.5])


# ---------------------------------------------------------------------------------- growth and reuse
def test_growth_and_upload_sequence_on_one_context():
    """One new context: a small long input (the long-entry and long-edge buffers grow from nothing and the
    split and the first-fit rerun), a full-block input with far more entries (they grow again), a short-only
    input (the virtual-read map must fall: fslr_long_query is a state error, the plain query gives the
    graph), the first input again (nothing of the larger queries may show) and the full-block input twice."""
    small, block = R.CASE['diag_65_65'], R.CASE['block_130_130_64']
    short = R.diagonal(40, 33)
    assert int(np.diff(short.csr().read_off).max()) <= _lib.FSLR_MAX_L
    c = _lib.Context(0)
    try:
        first = _abi_equals(c, small.data(), 0.8, [0.5])
        assert len(first[0]) == 1
        big = _abi_equals(c, block.data(), 0.8, [0.3])
        assert len(big[0]) == 3
        # long -> short-only
        idx = cluster.build_interval_trees(short, ctx=c)
        assert idx.long is None
        with pytest.raises(_lib.FslrError, match=ERR_STATE):
            c.long_query(QCUT, NCUT, pass_table([0.5]), 10)
        with pytest.raises(_lib.FslrError, match=ERR_STATE):
            c.set_long_cutoffs(umax_table([0.5], 130))
        want = R.long_ref(short.csr(), 0.8, [0.5])
        c.set_thresholds(fold_overlap_threshold(short.csr().iv_aln, 0.8))
        c.reserve_edges(1 << 16)
        st = c.run_query(QCUT, NCUT, pass_table([0.5]), 10)
        c.components()
        assert _sorted_edges(*c.edges(st['n_edges'])) == want.edges and len(want.edges) == 2
        np.testing.assert_array_equal(c.labels(), want.labels)
        np.testing.assert_array_equal(c.fwd_degree(), want.fwd)
        g = cluster.query_graph(idx, short, 0.8, [0.5], 10, R.QLEN_DIFF, R.NAL_DIFF)
        assert _sorted_edges(g.a, g.b, g.I, g.U) == want.edges
        # short-only -> long
        assert _abi_equals(c, small.data(), 0.8, [0.5]) == first
        assert _abi_equals(c, block.data(), 0.8, [0.3]) == big
        assert _abi_equals(c, block.data(), 0.8, [0.3]) == big
        idx = cluster.build_interval_trees(block.data(), ctx=c)
        _query_equals(idx, block.data(), 0.0, [0.3], block.ref(0.0, [0.3]), 'pairs')
        _query_equals(idx, block.data(), 0.8, [0.3], block.ref(0.8, [0.3]), 'sweep+long')
    finally:
        c.close()


def test_full_block_is_deterministic(ctx):
    """k_long_greedy appends its edges through an atomic counter: ten runs give the same sorted edges,
    forward degrees and labels."""
    case = R.CASE['block_130_130_64']
    data = case.data()
    idx = cluster.build_interval_trees(data, ctx=ctx)
    want = case.ref(0.8, [0.3])
    runs = []
    for _ in range(10):
        g = cluster.query_graph(idx, data, 0.8, [0.3], 10, R.QLEN_DIFF, R.NAL_DIFF)
        runs.append((_sorted_edges(g.a, g.b, g.I, g.U), g.fwd.tolist(), g.labels.tolist()))
    assert all(r == runs[0] for r in runs)
    assert runs[0] == (want.edges, want.fwd.tolist(), want.labels.tolist())
