"""Plain numpy / scipy statements of what the union-find and edge-list kernels compute on an arbitrary
graph (components.hip; cap.hip's fslr_cap_install_edges, fslr_sort_edges and the padded edge copies), and
the graph shapes the directed tests feed them.  Test infrastructure only: no GPU, nothing of the library.

Which rows each entry point ignores (min_labels applies the same rule):
  * fslr_components / fslr_local_forest take the context's edge list.  fslr_cap_install_edges drops the
    rows with a < 0 as it installs, so no negative end reaches the union; a self loop and a repeated edge
    are unions of one component with itself.
  * fslr_components_from_pairs skips a row with a < 0 or b < 0 (padding, (-1, -1) in practice); self loops
    and duplicates as above.
  * fslr_union_pairs (host or device pairs, or src == NULL: (k mod n, dst[k])) has no padding: every end
    must lie in [0, n).  Self loops (a read with its own label) and duplicates are no-ops.
"""
from __future__ import annotations

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

SHAPES = ('chain', 'chain_perm', 'star_low', 'star_high', 'two_chains_joined', 'ring', 'binary_tree', 'pairs',
          'critical', 'dense_small', 'dups_loops', 'empty')
ORDERS = ('generated', 'reversed', 'shuffled')


def _i64(x):
    return np.asarray(x, dtype=np.int64).reshape(-1)


def min_labels(n, a, b):
    """Label of each node 0 .. n-1: the smallest node of its connected component.  Rows with a negative
    end are dropped; self loops and duplicates change nothing."""
    a, b = _i64(a), _i64(b)
    keep = (a >= 0) & (b >= 0)
    a, b = a[keep], b[keep]
    assert a.size == 0 or (max(a.max(), b.max()) < n), 'an end outside [0, n)'
    g = coo_matrix((np.ones(a.size, np.int8), (a, b)), shape=(n, n))
    _, comp = connected_components(g, directed=False)
    mins = np.full(int(comp.max()) + 1 if n else 0, n, dtype=np.int64)
    np.minimum.at(mins, comp, np.arange(n))
    return mins[comp]


def forest_pairs(labels):
    """The (x, labels[x]) rows of the nodes that are not their own label, ascending x: [k, 2] int64."""
    lab = _i64(labels)
    x = np.flatnonzero(lab != np.arange(lab.size))
    return np.stack([x, lab[x]], axis=1)


def sorted_edges(a, b, iu):
    """The edge list grouped by a, each run in its previous order (a stable sort by a alone)."""
    a, b, iu = _i64(a), _i64(b), _i64(iu)
    o = np.argsort(a, kind='stable')
    return a[o], b[o], iu[o]


def installed(rows, n):
    """fslr_cap_install_edges of the [m, 4] rows {a, b, iu, -}: the rows with a >= 0 in row order (iu kept
    as 16 bits), the forward degrees bincount(a), the edge count and the largest forward degree."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    r = rows[rows[:, 0] >= 0]
    fwd = np.bincount(r[:, 0], minlength=n).astype(np.int64)
    return dict(a=r[:, 0], b=r[:, 1], iu=r[:, 2] & 0xffff, fwd=fwd, count=int(r.shape[0]),
                max_fwd=int(fwd.max()) if n else 0)


def padded_rows(cols, n_pad, pad):
    """The first n_pad rows of the columns ``cols`` stacked as [n_pad, len(cols)], short lists filled up
    with the row ``pad`` (what the padded device copies write)."""
    out = np.empty((n_pad, len(cols)), dtype=np.int64)
    out[:] = np.asarray(pad, dtype=np.int64)
    k = min(n_pad, len(cols[0]))
    for j, c in enumerate(cols):
        out[:k, j] = _i64(c)[:k]
    return out


def shape(name, n, seed):
    """The edge list (a, b) of one named shape on the nodes 0 .. n-1, as generated."""
    rng = np.random.default_rng([seed, n, SHAPES.index(name)])
    i = np.arange(n, dtype=np.int64)
    none = np.zeros(0, np.int64)
    if name == 'chain':                       # the path 0-1-...-(n-1)
        a, b = i[:-1], i[1:]
    elif name == 'chain_perm':                # a path through a random permutation of the ranks
        p = rng.permutation(n).astype(np.int64)
        a, b = p[:-1], p[1:]
    elif name == 'star_low':
        a, b = np.zeros(max(n - 1, 0), np.int64), i[1:]
    elif name == 'star_high':                 # every edge's larger end is the centre
        a, b = i[:-1], np.full(max(n - 1, 0), n - 1, np.int64)
    elif name == 'two_chains_joined':         # evens and odds, one last edge between their far ends
        ev, od = i[0::2], i[1::2]
        a = np.concatenate([ev[:-1], od[:-1], ev[-1:] if od.size else none])
        b = np.concatenate([ev[1:], od[1:], od[-1:]])
    elif name == 'ring':
        a = np.concatenate([i[:-1], i[-1:] if n >= 3 else none])
        b = np.concatenate([i[1:], i[:1] if n >= 3 else none])
    elif name == 'binary_tree':               # node k under (k - 1) // 2
        a, b = (i[1:] - 1) // 2, i[1:]
    elif name == 'pairs':                     # the perfect matching (2k, 2k + 1)
        a = 2 * np.arange(n // 2, dtype=np.int64)
        b = a + 1
    elif name == 'critical':                  # n / 2 uniformly random edges: the widest spread of sizes
        a, b = rng.integers(0, n, n // 2), rng.integers(0, n, n // 2)
    elif name == 'dense_small':               # the complete graph on the 24 highest ranks
        top = i[max(n - 24, 0):]
        x, y = np.triu_indices(top.size, 1)
        a, b = top[x], top[y]
    elif name == 'dups_loops':                # critical's edges three times in both orientations, n / 8 loops
        ca, cb = shape('critical', n, seed)
        loops = rng.integers(0, n, n // 8)
        a = np.concatenate([ca, cb] * 3 + [loops])
        b = np.concatenate([cb, ca] * 3 + [loops])
    elif name == 'empty':
        a, b = none, none
    else:
        raise KeyError(name)
    return _i64(a).copy(), _i64(b).copy()


def ordered(a, b, order, seed):
    """The list as generated, back to front, or shuffled with the seed."""
    if order == 'generated':
        return a, b
    if order == 'reversed':
        return a[::-1].copy(), b[::-1].copy()
    assert order == 'shuffled', order
    o = np.random.default_rng([seed, a.size, 7]).permutation(a.size)
    return a[o], b[o]


def shapes(n, seed, names=SHAPES):
    """(name, order, a, b) of every named shape in each of the three orders."""
    for name in names:
        a, b = shape(name, n, seed)
        for order in ORDERS:
            yield (name, order) + ordered(a, b, order, seed)
