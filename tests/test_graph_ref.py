"""tests/graph_ref.py (the scipy statement the GPU graph tests compare the kernels with) against three
independent answers on every shape and order: the project's host union-find, networkx, and its own
forest pairs fed back.  tests/sweep_emu.py's emulations of the same entry points (local_forest,
components_from_pairs, sort_edges, cap_install_edges, the padded copies, the label-vector union) are
pinned to it too, so the multi-process CPU tests of test_dist.py stand on a checked emulator."""
import types

import networkx as nx
import numpy as np
import pytest
import torch

import graph_ref as G
from fslr_amd.dist import union_find_labels
from sweep_emu import EmuSweepContext

SIZES = [1, 2, 257, 5000]
SEED = 20


@pytest.fixture(scope='module', params=SIZES)
def cases(request):
    n = request.param
    return n, [(name, order, a, b, G.min_labels(n, a, b)) for name, order, a, b in G.shapes(n, SEED)]


def test_every_shape_is_generated(cases):
    n, cs = cases
    assert [(c[0], c[1]) for c in cs] == [(s, o) for s in G.SHAPES for o in G.ORDERS]
    by = {(c[0], c[1]): c for c in cs}
    for name in G.SHAPES:
        a, b = by[name, 'generated'][2:4]
        for order in G.ORDERS:
            x, y = by[name, order][2:4]
            assert sorted(zip(x.tolist(), y.tolist())) == sorted(zip(a.tolist(), b.tolist())), (name, order)
            assert x.size == 0 or (0 <= min(x.min(), y.min()) and max(x.max(), y.max()) < n)
    # the shapes are what their names say
    sizes = {name: np.bincount(np.bincount(by[name, 'generated'][4])) for name in G.SHAPES}
    for name in ('chain', 'chain_perm', 'star_low', 'star_high', 'two_chains_joined', 'ring', 'binary_tree'):
        assert (by[name, 'generated'][4] == 0).all(), name                 # connected
        assert by[name, 'generated'][2].size == (n if name == 'ring' and n >= 3 else n - 1), name
    assert (by['pairs', 'generated'][4] == np.arange(n) // 2 * 2)[:n // 2 * 2].all()
    assert (by['empty', 'generated'][4] == np.arange(n)).all()
    assert (by['dups_loops', 'generated'][4] == by['critical', 'generated'][4]).all()
    assert by['dups_loops', 'generated'][2].size == 6 * (n // 2) + n // 8
    if n >= 24:
        assert sizes['dense_small'][24] == 1 and by['dense_small', 'generated'][2].size == 24 * 23 // 2
    if n == 5000:
        assert len(sizes['critical']) > 8 and sizes['critical'][1] > n // 4    # a spread of sizes, many singletons


def test_min_labels_equal_host_union_find(cases):
    n, cs = cases
    for name, order, a, b, want in cs:
        np.testing.assert_array_equal(want, union_find_labels(n, a, b), err_msg=f'{name} {order}')


def test_min_labels_equal_networkx(cases):
    n, cs = cases
    for name, order, a, b, want in cs:
        g = nx.Graph()
        g.add_nodes_from(range(n))
        g.add_edges_from(zip(a.tolist(), b.tolist()))
        lab = np.full(n, -1, np.int64)
        for comp in nx.connected_components(g):
            lab[list(comp)] = min(comp)
        np.testing.assert_array_equal(want, lab, err_msg=f'{name} {order}')


def test_forest_pairs_reproduce_the_labels(cases):
    n, cs = cases
    for name, order, a, b, want in cs:
        fp = G.forest_pairs(want)
        assert (np.diff(fp[:, 0]) > 0).all() and (fp[:, 1] < fp[:, 0]).all()
        assert fp.shape[0] == n - np.unique(want).size
        np.testing.assert_array_equal(G.min_labels(n, fp[:, 0], fp[:, 1]), want, err_msg=f'{name} {order}')


def test_negative_rows_are_dropped():
    a = np.array([0, -1, 2, 3, -1])
    b = np.array([1, -1, -1, 4, 2])
    np.testing.assert_array_equal(G.min_labels(5, a, b), [0, 0, 2, 3, 3])


def test_sorted_and_installed_statements():
    a = np.array([3, 1, 3, 0, 1, 3])
    b = np.array([9, 8, 7, 6, 5, 4])
    iu = np.arange(6)
    sa, sb, si = G.sorted_edges(a, b, iu)
    assert sa.tolist() == [0, 1, 1, 3, 3, 3] and sb.tolist() == [6, 8, 5, 9, 7, 4] and si.tolist() == [3, 1, 4, 0, 2, 5]
    rows = np.array([[-1, -1, 0, 0], [2, 0, 0x1ffff, 0], [-1, 5, 9, 0], [2, 1, 7, 0], [0, 3, 8, 0]])
    ins = G.installed(rows, 4)
    assert ins['a'].tolist() == [2, 2, 0] and ins['b'].tolist() == [0, 1, 3] and ins['iu'].tolist() == [0xffff, 7, 8]
    assert ins['fwd'].tolist() == [1, 0, 2, 0] and ins['count'] == 3 and ins['max_fwd'] == 2
    assert G.padded_rows((ins['a'], ins['b']), 5, (-1, -1)).tolist() == [[2, 0], [2, 1], [0, 3], [-1, -1], [-1, -1]]
    assert G.padded_rows((ins['a'], ins['b']), 2, (-1, -1)).tolist() == [[2, 0], [2, 1]]


# ---- the emulator of test_dist.py against the same statements ------------------------------------------
def _emu(n):
    csr = types.SimpleNamespace(n_reads=n, read_off=np.arange(n + 1), iv_chrom=np.zeros(n, np.int64),
                                data_pos=np.arange(n))
    return EmuSweepContext(csr, np.ones(n, np.int64))


def _rows_with_padding(a, b, rng):
    """{a, b, iu, 0} rows, iu = the edge's index, with nine padding rows at random places."""
    m = a.size
    pos = np.sort(rng.choice(m + 9, m, replace=False))
    rows = np.zeros((m + 9, 4), np.int32)
    rows[:, 0] = -1
    rows[:, 1] = -1
    rows[pos] = np.stack([a, b, np.arange(m) & 0xffff, np.zeros(m, np.int64)], axis=1)
    return rows


def test_emulator_equals_graph_ref(cases):
    n, cs = cases
    rng = np.random.default_rng(n)
    emu = _emu(n)
    for name, order, a, b, want in cs:
        msg = f'{name} {order}'
        rows = _rows_with_padding(a, b, rng)
        ins = G.installed(rows, n)
        emu.cap_install_edges(torch.from_numpy(rows.reshape(-1).copy()), rows.shape[0])
        ea, eb, eI, eU = emu.edges(ins['count'])
        np.testing.assert_array_equal(ea, ins['a'], err_msg=msg)
        np.testing.assert_array_equal(eb, ins['b'], err_msg=msg)
        np.testing.assert_array_equal(eI | (eU << 8), ins['iu'], err_msg=msg)
        np.testing.assert_array_equal(emu.fwd_degree(), ins['fwd'], err_msg=msg)
        # the padded copies
        for n_pad in {max(ins['count'] - 1, 0), ins['count'], ins['count'] + 5}:
            t = torch.zeros(n_pad, dtype=torch.int64)
            emu.edges_into(t, n_pad)
            np.testing.assert_array_equal(t.numpy().view(np.int32).reshape(-1, 2),
                                          G.padded_rows((ins['a'], ins['b']), n_pad, (-1, -1)), err_msg=msg)
            t = torch.zeros(4 * n_pad, dtype=torch.int32)
            emu.edges_iu_into(t, n_pad)
            np.testing.assert_array_equal(
                t.numpy().reshape(-1, 4),
                G.padded_rows((ins['a'], ins['b'], ins['iu'], np.zeros(ins['count'])), n_pad, (-1, -1, 0, 0)),
                err_msg=msg)
        # components, the forest and its pairs
        emu.components()
        np.testing.assert_array_equal(emu.labels(), want, err_msg=msg)
        fp = G.forest_pairs(want)
        k = emu.local_forest()
        assert k == fp.shape[0], msg
        for n_pad in {k, k + 7, max(k - 1, 0)}:
            t = torch.zeros(n_pad, dtype=torch.int64)
            emu.forest_pairs_into(t, n_pad)
            got = t.numpy().view(np.int32).reshape(-1, 2)
            np.testing.assert_array_equal(got, G.padded_rows((fp[:, 0], fp[:, 1]), n_pad, (-1, -1)), err_msg=msg)
        t = torch.from_numpy(rows[:, :2].copy().view(np.int64).reshape(-1))
        emu.components_from_pairs(t, rows.shape[0])              # the edges themselves, with their padding rows
        np.testing.assert_array_equal(emu.labels(), want, err_msg=msg)
        # the sort: stable by a
        emu.sort_edges()
        sa, sb, si = G.sorted_edges(ins['a'], ins['b'], ins['iu'])
        ea, eb, eI, eU = emu.edges(ins['count'])
        np.testing.assert_array_equal(ea, sa, err_msg=msg)
        np.testing.assert_array_equal(eb, sb, err_msg=msg)
        np.testing.assert_array_equal(eI | (eU << 8), si, err_msg=msg)
        # W = 3 partial labellings united
        emu.cap_install_edges(torch.zeros(0, dtype=torch.int32), 0)
        emu.components()
        parts = np.array_split(np.arange(a.size), 3)
        vec = np.concatenate([G.min_labels(n, a[p], b[p]) for p in parts]).astype(np.int32)
        emu.union_label_vectors(torch.from_numpy(vec))
        np.testing.assert_array_equal(emu.labels(), want, err_msg=msg)
