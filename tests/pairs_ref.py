"""Plain reference for the sweep engine's pair evaluation (fslr_sweep_evaluate), and builders for
its input.  Test infrastructure only; not a test module.

The operation: the caller hands over match entries, one per interval pair (interval i of read A,
interval j of read B, A < B read ranks) that passed the overlap test.  Per read pair the reference's
overall_jaccard_similarity (cluster.py:140-170) walks A's intervals in order and gives each the first
interval of B, in order, that matches it and that no earlier interval of A took; I is the number of
intervals of A that found one and U = L_A + L_B - I.  The pair is an edge iff I > 0 and
I / U >= jaccard_threshold[min(I, len) - 1] in Python floats (cluster.py:216-219).

Written from those lines of the reference, not from the device kernels or their host emulation
(tests/sweep_emu.py), which the tests use as a second opinion.
"""
from collections import namedtuple

import numpy as np

A_SHIFT, B_SHIFT, I_SHIFT = 39, 14, 7          # entry = A << 39 | B << 14 | i << 7 | j (fslr_hip.h)
RANK_MASK = (1 << 25) - 1
MAX_L = 64


def pack(a, b, i, j):
    a, b, i, j = (np.asarray(x, dtype=np.int64) for x in (a, b, i, j))
    return (a << A_SHIFT) | (b << B_SHIFT) | (i << I_SHIFT) | j


def unpack(entries):
    e = np.asarray(entries, dtype=np.int64)
    return e >> A_SHIFT, (e >> B_SHIFT) & RANK_MASK, (e >> I_SHIFT) & 127, e & 127


def first_fit(cells):
    """I of one read pair from its matching (i, j) cells: cluster.py:152-161 with the overlap test
    replaced by membership in ``cells``."""
    rows = {}
    for i, j in cells:
        rows.setdefault(int(i), []).append(int(j))
    taken = set()
    intersection = 0
    for i in sorted(rows):                      # for i, interval1 in enumerate(l1)
        for j in sorted(rows[i]):               # for j, interval2 in enumerate(l2): the matching ones
            if j in taken:                      # if l2_comparisons[j]: continue
                continue
            taken.add(j)
            intersection += 1
            break
    return intersection


def evaluate_entries(entries, read_len, cutoffs):
    """``(edges, fwd, n_pairs)``: edges the sorted list of (A, B, I, U), fwd[A] the edges of A as the
    lower read (int64[n_reads]), n_pairs the distinct (A, B) among the entries."""
    L = np.asarray(read_len, dtype=np.int64)
    cut = [float(c) for c in cutoffs]
    fwd = np.zeros(L.size, np.int64)
    a, b, i, j = unpack(entries)
    pairs = {}
    for x, y, r, c in zip(a.tolist(), b.tolist(), i.tolist(), j.tolist()):
        pairs.setdefault((x, y), []).append((r, c))
    edges = []
    for (x, y), cells in pairs.items():
        I = first_fit(cells)
        U = int(L[x] + L[y]) - I
        if I == 0:
            continue
        target = cut[I - 1] if I - 1 < len(cut) else cut[-1]
        if I / U >= target:
            edges.append((x, y, I, U))
            fwd[x] += 1
    return sorted(edges), fwd, len(pairs)


def pair_intersections(entries):
    """{(A, B): (I, entry count)} of every pair among the entries."""
    a, b, i, j = unpack(entries)
    pairs = {}
    for x, y, r, c in zip(a.tolist(), b.tolist(), i.tolist(), j.tolist()):
        pairs.setdefault((x, y), []).append((r, c))
    return {k: (first_fit(v), len(v)) for k, v in pairs.items()}


def build_entries(desc, read_len, seed=0):
    """The entry set of a description ``[(A, B, cells), ...]``, cells an (m, 2) array-like of (i, j);
    a pair may be listed once.  Asserts what the kernel requires of its input (A < B < n_reads,
    i < L_A, j < L_B, L <= 64, no entry twice) and returns the entries in a seeded random order: the
    grouping must not depend on the order they arrive in."""
    L = np.asarray(read_len, dtype=np.int64)
    assert L.size == 0 or (1 <= L.min() and L.max() <= MAX_L)
    parts = []
    seen = set()
    for A, B, cells in desc:
        c = np.asarray(cells, dtype=np.int64).reshape(-1, 2)
        assert 0 <= A < B < L.size, (A, B, L.size)
        assert (A, B) not in seen, (A, B)
        seen.add((A, B))
        assert c.shape[0] > 0
        assert c[:, 0].min() >= 0 and c[:, 0].max() < L[A], (A, B)
        assert c[:, 1].min() >= 0 and c[:, 1].max() < L[B], (A, B)
        parts.append(pack(A, B, c[:, 0], c[:, 1]))
    ent = np.concatenate(parts) if parts else np.zeros(0, np.int64)
    assert np.unique(ent).size == ent.size, 'an entry twice'
    return ent[np.random.default_rng(seed).permutation(ent.size)]


def union_find_labels(n, edges):
    """label[v] = the smallest read of v's component over ``edges`` [(A, B, ...)]."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for e in edges:
        x, y = find(e[0]), find(e[1])
        if x != y:
            parent[max(x, y)] = min(x, y)
    return np.array([find(v) for v in range(n)], dtype=np.int64)


# ---------------------------------------------------------------------------------- cell patterns
def cells(rng, la, lb, m, kind, ilo=0, ihi=None, jlo=0, jhi=None):
    """``m`` distinct cells of the la x lb match matrix, rows in [ilo, ihi), columns in [jlo, jhi):
    'perm'  no two share a row or a column (I = m);
    'row'   columns all different, rows repeat (I = the distinct rows);
    'col'   rows all different, columns repeat;
    'both'  a random subset of a small box: rows and columns repeat;
    'full'  the whole box."""
    ihi = la if ihi is None else min(ihi, la)
    jhi = lb if jhi is None else min(jhi, lb)
    ni, nj = ihi - ilo, jhi - jlo
    assert ni > 0 and nj > 0
    if kind == 'full':
        ii, jj = np.divmod(np.arange(ni * nj), nj)
    elif kind == 'perm':
        assert m <= min(ni, nj), (m, ni, nj)
        ii, jj = rng.permutation(ni)[:m], rng.permutation(nj)[:m]
    elif kind == 'row':
        assert m <= nj, (m, nj)
        jj = rng.permutation(nj)[:m]
        ii = rng.integers(0, max(1, min(ni, (m + 1) // 2)), m)
    elif kind == 'col':
        assert m <= ni, (m, ni)
        ii = rng.permutation(ni)[:m]
        jj = rng.integers(0, max(1, min(nj, (m + 1) // 2)), m)
    elif kind == 'both':
        side = int(np.ceil(np.sqrt(m))) + 1
        r, c = min(ni, side), min(nj, side)
        while r * c < m:                        # a box too narrow on one side grows on the other
            if r < ni and (r <= c or c == nj):
                r += 1
            else:
                assert c < nj, (m, ni, nj)
                c += 1
        ii, jj = np.divmod(rng.permutation(r * c)[:m], c)
    else:
        raise ValueError(kind)
    return np.stack([ii + ilo, jj + jlo], axis=1)


# ---------------------------------------------------------------------------------- KATs
_Itv = namedtuple('_Itv', ['chrom', 'start', 'end', 'aln_size'])


def kat_cells(k, calculate_overlap):
    """The matching (i, j) of a golden Jaccard KAT (lists 'a' and 'b' of (chrom, start, end, aln_size),
    cutoff 'pct'): same chromosome and calculate_overlap >= pct (cluster.py:157)."""
    l1 = [_Itv(*x) for x in k['a']]
    l2 = [_Itv(*x) for x in k['b']]
    return [(i, j) for i, x in enumerate(l1) for j, y in enumerate(l2)
            if x.chrom == y.chrom and calculate_overlap(x, y) >= k['pct']]
