"""The union-find (components.hip) and the edge-list kernels of cap.hip (fslr_cap_install_edges,
fslr_sort_edges, the padded copies) on arbitrary graphs, compared exactly with tests/graph_ref.py.

The context holds n reads of one interval each on one chromosome, with starts that do not overlap: no
index is built and no query runs (one case excepted), so a graph reaches the kernels only through
cap_install_edges or as pairs.  Every end fed to the device lies in [0, n), apart from the documented
(-1, -1) padding rows.

Cost bound of the deep shapes (a condition checked before the first device run, not a measurement).
components.hip, for a path of n reads: k_uf_hook_min makes p[x] = the smallest neighbour below x, for
the chain 0-1-...-(n-1) p[x] = x - 1, a tree of depth n - 1, the deepest there is.  k_uf_edges then runs
one uf_union per edge; its two uf_find walks go up from x two levels per iteration at two loads per
iteration, so they cost at most depth(x) + 1 dependent loads each whether or not the halving stores land,
and a failed CAS continues from the fresh parent, strictly upwards, so the retries of one union add at
most one more walk.  With no compression at all the walks of the n - 1 edges sum to
1 + 2 + ... + (n - 1) ~ n^2 / 2 dependent loads, and k_uf_finalize / k_forest_count (uf_root, no
halving by design) are bounded by the same sum.  Taking the worst case that one thread runs them all,
at one load per 2 us, a pass takes n^2 / 2 * 2 us = n^2 us: under 10 s needs n <= 3162.  DEEP_N = 3161
is the largest such size that is odd and no multiple of the wavefront or the block.  (The kernels spread
the edges over up to 2^20 threads, one edge each at these sizes, so one thread's dependent chain is a few
walks, <= ~4 n loads = 25 ms by the same rate: the bound is the serial worst case.)  The sizes the cases
share, up to 4097, give 17 s per pass by this bound; the file is run under a time limit of 600 s, and a case
that reached it would be read from the code, not rerun.
"""
import numpy as np
import pytest
import torch

import graph_ref as G
from fslr_amd import _lib, synth
from fslr_amd.prep import fold_overlap_threshold, pass_table

pytestmark = pytest.mark.gpu

SEED = 23
SIZES = [1, 2, 63, 64, 65, 257, 4097]
DEEP_N = 3161                                     # n^2 us <= 10 s (the derivation above)
DEEP_SHAPES = ('chain', 'chain_perm', 'two_chains_joined')
SENTINEL = 0x5a5a5a5a


class Graphs:
    """One context whose reads are replaced when n changes; its edge list starts empty."""

    def __init__(self):
        self.ctx = _lib.Context(0)
        self.n = None

    def reads(self, n):
        if self.n != n:
            i = np.arange(n)
            one = np.ones(n, np.int32)
            self.ctx.set_reads(np.arange(n + 1), one, one, np.zeros(n, np.int32), 10 * i, 10 * i + 5, one, 1)
            self.n = n
            install(self.ctx, np.zeros((0, 4), np.int32))
        return self.ctx


@pytest.fixture(scope='module')
def gr():
    g = Graphs()
    yield g
    g.ctx.close()


@pytest.fixture(scope='module')
def gr2():
    g = Graphs()
    yield g
    g.ctx.close()


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to('cuda:0')


def filled(count, dtype):
    """A device tensor of SENTINEL words, complete before the context's own stream writes into it."""
    t = torch.full((count,), SENTINEL, dtype=dtype, device='cuda:0')
    torch.cuda.synchronize()
    return t


def rows_of(a, b, iu=None):
    rows = np.zeros((len(a), 4), np.int32)
    rows[:, 0] = a
    rows[:, 1] = b
    rows[:, 2] = 0 if iu is None else iu
    return rows


def install(ctx, rows):
    ctx.cap_install_edges(dev(rows.reshape(-1)), rows.shape[0])       # syncs


def device_edges(ctx):
    k = ctx.stats()['n_edges']
    a, b, I, U = ctx.edges(k)
    return a, b, I | (U << 8)


def pairs_with_padding(a, b, rng):
    """(a, b) int32 rows with (-1, -1) rows at random places (about one in eight, at least three)."""
    m, pad = a.size, max(3, a.size // 8)
    pos = np.sort(rng.choice(m + pad, m, replace=False))
    out = np.full((m + pad, 2), -1, np.int32)
    out[pos, 0] = a
    out[pos, 1] = b
    return out


def check_every_route(g, n, name, order, a, b, rng):
    """The four union kernels (k_uf_edges, k_uf_pair_list, k_uf_pairs from host pairs, k_uf_pairs with
    src == NULL) on one edge list: each gives min_labels of the whole list."""
    ctx = g.reads(n)
    want = G.min_labels(n, a, b)
    msg = f'{name} {order} n={n}'
    # 1: the context's edges
    install(ctx, rows_of(a, b))
    ctx.components()
    np.testing.assert_array_equal(ctx.labels(), want, err_msg=f'components: {msg}')
    # 2: a pair list with padding rows
    t = dev(pairs_with_padding(a, b, rng).reshape(-1))
    ctx.components_from_pairs(t, t.numel() // 2)
    np.testing.assert_array_equal(ctx.labels(), want, err_msg=f'components_from_pairs: {msg}')
    # 3: host pairs into the identity forest
    install(ctx, np.zeros((0, 4), np.int32))
    ctx.components()
    np.testing.assert_array_equal(ctx.labels(), np.arange(n), err_msg=f'no edges: {msg}')
    if a.size:
        ctx.union_pairs(a, b, a.size, on_device=False)
    ctx.finalize_labels()
    np.testing.assert_array_equal(ctx.labels(), want, err_msg=f'union_pairs: {msg}')
    # 4: W = 3 stacked label vectors, each the labelling of a third of the edges (src == NULL)
    ctx.components()
    vec = np.concatenate([G.min_labels(n, a[p], b[p]) for p in np.array_split(np.arange(a.size), 3)])
    t = dev(vec.astype(np.int32))
    ctx.union_label_vectors(t)
    np.testing.assert_array_equal(ctx.labels(), want, err_msg=f'union_label_vectors: {msg}')


@pytest.mark.parametrize('name', G.SHAPES)
@pytest.mark.parametrize('n', SIZES)
def test_components_through_every_union_kernel(gr, n, name):
    rng = np.random.default_rng([SEED, n])
    a0, b0 = G.shape(name, n, SEED)
    for order in G.ORDERS:
        a, b = G.ordered(a0, b0, order, SEED)
        check_every_route(gr, n, name, order, a, b, rng)


@pytest.mark.parametrize('name', DEEP_SHAPES)
def test_deep_shapes_at_the_cost_bound(gr, name):
    rng = np.random.default_rng([SEED, DEEP_N])
    a0, b0 = G.shape(name, DEEP_N, SEED)
    for order in G.ORDERS:
        a, b = G.ordered(a0, b0, order, SEED)
        check_every_route(gr, DEEP_N, name, order, a, b, rng)


@pytest.mark.parametrize('name,order', [('star_high', 'generated'), ('chain', 'reversed'), ('critical', 'generated')])
def test_labels_stable_over_repeats(gr, name, order):
    """20 components() calls on shapes with contention (every atomicMin of the star on one word) and depth
    (a path hooked into a tree of depth n - 1): k_uf_finalize must not race with a halving store."""
    n = 4097
    ctx = gr.reads(n)
    a, b = G.ordered(*G.shape(name, n, SEED), order, SEED)
    want = G.min_labels(n, a, b)
    install(ctx, rows_of(a, b))
    for rep in range(20):
        ctx.components()
        np.testing.assert_array_equal(ctx.labels(), want, err_msg=f'repeat {rep}')


# chunk = max(256, ceil(n / 1024)): 256 up to n = 262144 (1, 2, 1023 and 1024 blocks), then 257 (a partial last
# iteration of k_forest_write in every block)
FOREST_SIZES = [1, 255, 256, 257, 511, 513, 262143, 262144, 262145, 262147 + 256]


@pytest.mark.parametrize('name', ['pairs', 'star_low', 'critical', 'empty'])
@pytest.mark.parametrize('n', FOREST_SIZES)
def test_forest_pair_list(gr, gr2, n, name):
    """fslr_local_forest's list itself: the (read, root) pairs of the non-root reads in read order, their
    count, the (-1, -1) padding of the copy, the finalized labels, and the union of the copied pairs."""
    ctx = gr.reads(n)
    a, b = G.shape(name, n, SEED)
    want = G.min_labels(n, a, b)
    fp = G.forest_pairs(want)
    install(ctx, rows_of(a, b))
    k = ctx.local_forest()
    assert k == fp.shape[0]
    np.testing.assert_array_equal(ctx.labels(), want)                 # the forest call finalizes
    for n_pad in sorted({k, k + 7} | ({k - 1} if k > 0 else set())):
        t = filled(n_pad + 1, torch.int64)
        ctx.forest_pairs_into(t, n_pad)
        ctx.sync()
        got = t.cpu().numpy()
        assert got[n_pad] == SENTINEL                                  # nothing past n_pad pairs
        np.testing.assert_array_equal(got[:n_pad].view(np.int32).reshape(-1, 2),
                                      G.padded_rows((fp[:, 0], fp[:, 1]), n_pad, (-1, -1)), err_msg=f'n_pad={n_pad}')
        if n_pad == k + 7:
            c2 = gr2.reads(n)
            c2.components_from_pairs(t, n_pad)
            np.testing.assert_array_equal(c2.labels(), want)


def test_installed_graph_after_a_pre_hooked_sweep():
    """A sweep query pre-hooks the parents as it forms edges; installing another graph afterwards
    (cap_work clears the hook) must give the labels of the installed graph alone."""
    s = synth.generate(3000, 16, 11)
    csr = s.interval_data().csr()
    n = csr.n_reads
    ctx = _lib.Context(0)
    try:
        ctx.load_csr(csr, fold_overlap_threshold(csr.iv_aln, 0.8))
        ctx.reserve_edges(12 * n)
        ctx.build_index()
        ctx.query(1 - 0.04, 1 - 0.25, pass_table([1, 1, 0.66, 0.66, 0.66, 0.5]), 10, engine='sweep')
        st = ctx.stats()
        assert st['engine'] == 'sweep' and 0 < st['n_edges']
        oa, ob, _, _ = ctx.edges(st['n_edges'])
        a, b = G.shape('pairs', n, SEED)
        assert a.size <= st['edge_capacity']                          # no reallocation on the way
        want = G.min_labels(n, a, b)
        # the sweep's own edges join reads the installed graph keeps apart: a hook left standing would show
        assert (want[oa] != want[ob]).any()
        install(ctx, rows_of(a, b))
        assert ctx.stats()['edge_capacity'] == st['edge_capacity']
        ctx.components()
        np.testing.assert_array_equal(ctx.labels(), want)
    finally:
        ctx.close()


def sort_case(name, n):
    """The shape's edges plus edges whose lower read is n - 1 or n - 2 (the top of the key range), shuffled,
    with iu = the row's index so that every row is identifiable."""
    rng = np.random.default_rng([SEED, n, 99])
    a, b = G.shape(name, n, SEED)
    top = np.concatenate([np.full(5, n - 1), np.full(4, n - 2)])
    a = np.concatenate([a, top])
    b = np.concatenate([b, rng.integers(0, n, top.size)])
    o = rng.permutation(a.size)
    a, b = a[o], b[o]
    return a, b, np.arange(a.size) & 0xffff


@pytest.mark.parametrize('name', ['critical', 'dups_loops'])
@pytest.mark.parametrize('n', [2, 256, 257, 4096, 4097, 65536, 65537])
def test_sort_edges_is_stable_and_carries_iu(gr, n, name):
    ctx = gr.reads(n)
    a, b, iu = sort_case(name, n)
    want = G.min_labels(n, a, b)
    install(ctx, rows_of(a, b, iu))
    ctx.sort_edges()
    sa, sb, si = G.sorted_edges(a, b, iu)
    ga, gb, gi = device_edges(ctx)
    np.testing.assert_array_equal(ga, sa)
    np.testing.assert_array_equal(gb, sb)                             # the order inside each run
    np.testing.assert_array_equal(gi, si)
    np.testing.assert_array_equal(ctx.fwd_degree(), np.bincount(a, minlength=n))
    ctx.components()
    np.testing.assert_array_equal(ctx.labels(), want)


@pytest.mark.parametrize('m', [0, 1])
def test_sort_edges_of_at_most_one_edge_is_a_no_op(gr, m):
    n = 257
    ctx = gr.reads(n)
    rows = rows_of([n - 1] * m, [3] * m, [0x1234] * m)
    install(ctx, rows)
    ctx.sort_edges()
    ga, gb, gi = device_edges(ctx)
    assert (ga.tolist(), gb.tolist(), gi.tolist()) == ([n - 1] * m, [3] * m, [0x1234] * m)


def padded_install_rows(n, rng):
    """Rows of dups_loops with padding (a = -1) at the front, at the back, in runs and alone."""
    a, b = G.shape('dups_loops', n, SEED)
    o = rng.permutation(a.size)
    a, b = a[o], b[o]
    pad = np.zeros(a.size + 1, np.int64)                             # padding rows before edge k (the last: the back)
    pad[0] = 5
    pad[-1] = 3
    pad[a.size // 2] = 300                                           # a run longer than a block
    pad[rng.choice(np.arange(1, a.size), a.size // 7, replace=False)] += 1
    pos = np.cumsum(pad[:-1]) + np.arange(a.size)
    rows = np.zeros((a.size + int(pad.sum()), 4), np.int32)
    rows[:, 0] = -1
    rows[:, 1] = rng.integers(-1, n, rows.shape[0])                  # a < 0 alone marks a padding row
    rows[pos, 0] = a
    rows[pos, 1] = b
    rows[pos, 2] = (pos * 7 + 1) & 0xffff
    return rows


def check_padded_copies(ctx, ins):
    cnt = ins['count']
    for n_pad in sorted({max(cnt - 3, 0), cnt, cnt + 5}):
        t = filled(2 * (n_pad + 1), torch.int32)
        ctx.edges_into(t, n_pad)
        t4 = filled(4 * (n_pad + 1), torch.int32)
        ctx.edges_iu_into(t4, n_pad)
        ctx.sync()
        got, got4 = t.cpu().numpy().reshape(-1, 2), t4.cpu().numpy().reshape(-1, 4)
        assert (got[n_pad] == SENTINEL).all() and (got4[n_pad] == SENTINEL).all()
        np.testing.assert_array_equal(got[:n_pad], G.padded_rows((ins['a'], ins['b']), n_pad, (-1, -1)))
        np.testing.assert_array_equal(
            got4[:n_pad], G.padded_rows((ins['a'], ins['b'], ins['iu'], np.zeros(cnt)), n_pad, (-1, -1, 0, 0)))


@pytest.mark.parametrize('n', [65, 4097])
def test_install_compacts_padding_and_copies_pad(gr, n):
    ctx = gr.reads(n)
    rows = padded_install_rows(n, np.random.default_rng([SEED, n, 5]))
    ins = G.installed(rows, n)
    assert 0 < ins['count'] < rows.shape[0] and rows[0, 0] < 0 and rows[-1, 0] < 0
    install(ctx, rows)
    ga, gb, gi = device_edges(ctx)
    np.testing.assert_array_equal(ga, ins['a'])
    np.testing.assert_array_equal(gb, ins['b'])
    np.testing.assert_array_equal(gi, ins['iu'])
    np.testing.assert_array_equal(ctx.fwd_degree(), ins['fwd'])
    st = ctx.stats()
    assert (st['n_edges'], st['max_fwd']) == (ins['count'], ins['max_fwd'])
    check_padded_copies(ctx, ins)
    ctx.components()
    np.testing.assert_array_equal(ctx.labels(), G.min_labels(n, ins['a'], ins['b']))
    # only padding, then no rows at all: an empty list and zero degrees
    for empty in (np.full((300, 4), -1, np.int32), np.zeros((0, 4), np.int32)):
        install(ctx, empty)
        ins0 = G.installed(empty, n)
        st = ctx.stats()
        assert (st['n_edges'], st['max_fwd']) == (0, 0)
        np.testing.assert_array_equal(ctx.fwd_degree(), np.zeros(n))
        check_padded_copies(ctx, ins0)
        ctx.components()
        np.testing.assert_array_equal(ctx.labels(), np.arange(n))


def test_union_pairs_without_reads_is_refused():
    """src == NULL means k mod n_reads: refused on a context without reads, before any device temporary is
    made, and the context works afterwards."""
    g = Graphs()
    try:
        for on_device in (False, True):
            with pytest.raises(_lib.FslrError, match=f'fslr error {_lib.FSLR_ERR_INVALID}: no reads'):
                if on_device:
                    t = dev(np.zeros(4, np.int32))
                    g.ctx.union_pairs(None, t.data_ptr(), 4, on_device=True)
                else:
                    g.ctx.union_pairs(None, np.zeros(4, np.int32), 4, on_device=False)
        ctx = g.reads(65)
        a, b = G.shape('ring', 65, SEED)
        ctx.components()
        ctx.union_pairs(a, b, a.size, on_device=False)
        ctx.finalize_labels()
        np.testing.assert_array_equal(ctx.labels(), np.zeros(65))
    finally:
        g.ctx.close()
