"""The pair-evaluation reference of the directed sweep tests (tests/pairs_ref.py) pinned on the CPU:
hand-computed first-fit patterns, the host emulation of fslr_sweep_evaluate as a second opinion, and
the reference's golden Jaccard KATs."""
import types

import numpy as np
import pytest

import fixtures as fx
import pairs_ref as pr
from fslr_amd import cluster
from fslr_amd.prep import pass_table

CUTS = (1, 1, 0.66, 0.66, 0.66, 0.5)


@pytest.mark.parametrize('cells,want', [
    ([(0, 0), (0, 1), (1, 0)], 1),            # row 0 takes column 0, row 1 has nothing left: below the maximum matching (2)
    ([(0, 1), (1, 0), (1, 1)], 2),            # row 0 takes 1, row 1 takes 0
    ([(0, 2), (0, 5), (0, 7)], 1),            # one row, three columns
    ([(3, 1), (3, 4), (5, 0), (5, 6)], 2),    # rows repeat, columns all different: I = rows
    ([(2, 4), (3, 4), (9, 4)], 1),            # one column, three rows
    ([(0, 1), (1, 1), (2, 3), (4, 3)], 2),    # columns repeat, rows all different: I = columns
    ([(0, 0), (1, 0), (1, 1), (2, 1), (2, 2)], 3),   # each row pushed to its second column
    ([(0, 1), (1, 1), (2, 0), (2, 1)], 2),    # row 1 finds column 1 taken; row 2 takes 0
    ([(5, 63)], 1),
])
def test_first_fit_by_hand(cells, want):
    assert pr.first_fit(cells) == want
    assert pr.first_fit(cells[::-1]) == want          # the order the cells arrive in is irrelevant


def test_first_fit_full_block():
    full = [(i, j) for i in range(64) for j in range(64)]
    assert pr.first_fit(full) == 64
    assert pr.first_fit([(i, j) for i in range(64) for j in range(3)]) == 3
    assert pr.first_fit([(i, j) for i in range(2) for j in range(64)]) == 2


def test_evaluate_entries_by_hand():
    """Three reads of 3, 2 and 64 intervals.  (0, 1): cells {(0,0),(0,1),(1,0)}: I = 1, U = 4, 1/4 < 1;
    (0, 2): a diagonal of 3: I = 3, U = 64, 3/64 < 0.66; (1, 2): {(0,5),(1,5)}: I = 1, U = 65."""
    L = [3, 2, 64]
    desc = [(0, 1, [(0, 0), (0, 1), (1, 0)]), (0, 2, [(0, 0), (1, 1), (2, 2)]), (1, 2, [(0, 5), (1, 5)])]
    ent = pr.build_entries(desc, L, seed=3)
    assert sorted(ent.tolist()) == sorted(
        (a << 39) | (b << 14) | (i << 7) | j for a, b, c in desc for i, j in c)
    edges, fwd, n_pairs = pr.evaluate_entries(ent, L, [0.0])
    assert edges == [(0, 1, 1, 4), (0, 2, 3, 64), (1, 2, 1, 65)]
    assert fwd.tolist() == [2, 1, 0] and n_pairs == 3
    edges, fwd, n_pairs = pr.evaluate_entries(ent, L, CUTS)
    assert edges == [] and fwd.tolist() == [0, 0, 0] and n_pairs == 3
    # the cut is indexed by I and clamps to the last entry: I = 3 > len([.5, .04]) reads 0.04 <= 3/64
    edges, fwd, _ = pr.evaluate_entries(ent, L, [0.5, 0.04])
    assert edges == [(0, 2, 3, 64)] and fwd.tolist() == [1, 0, 0]
    edges, fwd, n_pairs = pr.evaluate_entries(np.zeros(0, np.int64), L, CUTS)
    assert edges == [] and fwd.tolist() == [0, 0, 0] and n_pairs == 0
    assert pr.union_find_labels(4, [(1, 3, 1, 1), (0, 3, 1, 1)]).tolist() == [0, 0, 2, 0]


@pytest.mark.parametrize('bad', [
    [(1, 1, [(0, 0)])],                       # A == B
    [(2, 1, [(0, 0)])],                       # A > B
    [(0, 3, [(0, 0)])],                       # B >= n_reads
    [(0, 1, [(3, 0)])],                       # i >= L_A
    [(0, 1, [(0, 2)])],                       # j >= L_B
    [(0, 1, [(0, 0), (0, 0)])],               # an entry twice
    [(0, 1, [(0, 0)]), (0, 1, [(1, 1)])],     # a pair twice
])
def test_build_entries_refuses_what_the_kernel_does_not_take(bad):
    with pytest.raises(AssertionError):
        pr.build_entries(bad, [3, 2, 64])


def test_build_entries_shuffles():
    desc = [(0, 1, [(i, i) for i in range(40)])]
    L = [64, 64]
    e0, e1 = pr.build_entries(desc, L, seed=0), pr.build_entries(desc, L, seed=1)
    assert sorted(e0.tolist()) == sorted(e1.tolist()) and e0.tolist() != e1.tolist()
    assert e0.tolist() != sorted(e0.tolist())


@pytest.mark.parametrize('kind', ['perm', 'row', 'col', 'both', 'full'])
def test_cell_patterns(kind):
    rng = np.random.default_rng(5)
    for la, lb, m, box in [(64, 64, 1, {}), (64, 64, 30, {}), (40, 56, 25, {}),
                           (64, 64, 20, dict(ilo=32, jlo=32)), (64, 64, 20, dict(ihi=32, jhi=32))]:
        c = pr.cells(rng, la, lb, m, kind, **box)
        if kind != 'full':
            assert c.shape == (m, 2)
        assert len({tuple(x) for x in c.tolist()}) == c.shape[0]
        assert c[:, 0].min() >= box.get('ilo', 0) and c[:, 0].max() < min(la, box.get('ihi', la))
        assert c[:, 1].min() >= box.get('jlo', 0) and c[:, 1].max() < min(lb, box.get('jhi', lb))
        rows, cols = np.unique(c[:, 0]).size, np.unique(c[:, 1]).size
        I = pr.first_fit(c.tolist())
        if kind == 'perm':
            assert rows == cols == I == m
        if kind == 'row':
            assert cols == m and I == rows and (m == 1 or rows < m)
        if kind == 'col':
            assert rows == m and (m == 1 or cols < m) and I <= cols
        if kind == 'full':
            assert I == min(rows, cols)


def _random_entries(seed):
    rng = np.random.default_rng(seed)
    n = 40
    L = rng.integers(1, 65, n)
    desc = []
    for a in range(n - 1):
        for b in rng.choice(np.arange(a + 1, n), size=min(n - 1 - a, int(rng.integers(0, 6))), replace=False):
            box = int(L[a]) * int(L[b])
            m = int(rng.choice([1, max(1, box // 16), max(1, box // 2), box]))
            flat = rng.permutation(box)[:m]
            desc.append((a, int(b), np.stack(np.divmod(flat, int(L[b])), axis=1)))
    return L, pr.build_entries(desc, L, seed)


@pytest.mark.parametrize('seed', range(20))
def test_agrees_with_the_host_emulation(seed):
    """sweep_emu.EmuSweepContext.sweep_evaluate (the multi-GPU tests' stand-in for the device) on
    random entry sets: the same edges, forward degrees and edge count, under both cut tables."""
    import torch
    from sweep_emu import EmuSweepContext
    L, ent = _random_entries(seed)
    off = np.concatenate([[0], np.cumsum(L)])
    emu = EmuSweepContext(types.SimpleNamespace(n_reads=L.size, read_off=off, data_pos=np.arange(off[-1]),
                                                iv_chrom=np.zeros(off[-1], np.int64)), np.ones(off[-1], np.int64))
    differ = 0
    for cut in ([0.0], CUTS):
        edges, fwd, _ = pr.evaluate_entries(ent, L, cut)
        emu.sweep_evaluate(1.0, 1.0, pass_table(cut), torch.from_numpy(ent), ent.size)
        a, b, I, U = emu.edges(emu.stats()['n_edges'])
        assert sorted(zip(a.tolist(), b.tolist(), I.tolist(), U.tolist())) == edges
        np.testing.assert_array_equal(emu.fwd_degree(), fwd)
        differ += sum(I != m for I, m in pr.pair_intersections(ent).values())
    assert differ > 0


def test_golden_jaccard_kats():
    """Every golden KAT of overall_jaccard_similarity whose intervals all have aln_size > 0 (the
    reference divides by it): entries from cluster.calculate_overlap, then I == n_i and I / U == j."""
    kats = [k for k in fx.kats()['jaccard'] if 'raises' not in k]
    checked = conflicts = 0
    for k in kats:
        if any(x[3] == 0 for x in k['a'] + k['b']):
            continue
        c = pr.kat_cells(k, cluster.calculate_overlap)
        I = pr.first_fit(c)
        assert I == k['n_i'], k
        U = len(k['a']) + len(k['b']) - I
        assert (I / U if U else 0) == k['j'], k
        if c:
            L = [len(k['a']), len(k['b'])]
            edges, fwd, n_pairs = pr.evaluate_entries(pr.build_entries([(0, 1, c)], L), L, [0.0])
            assert edges == ([(0, 1, I, U)] if I else []) and n_pairs == 1
        checked += 1
        conflicts += I != len(c)
    assert checked > 2500 and conflicts > 0, (checked, conflicts)
