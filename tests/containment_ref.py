"""The plain statement of the path containment (include/fslr_hip.h fslr_cluster_path_containment), on the host, on the
dict that tests/paths_ref.py's ``paths`` returns.

Row A has the tokens A[0..a-1], t = locus * 2 + rev; rc(A) is A reversed with every low bit flipped.  A is contained
in B iff they lie in one cluster, a < b, and B[o:o + a] equals A (d = 0) or rc(A) (d = 1) for some offset o; every
such (o, d) is an occurrence, and for a palindromic A (rc(A) == A) only d = 0 counts.  Brute force: every ordered
pair of a cluster's rows, every offset, both directions; no anchor, no index.
tests/test_containment_ref.py pins it to hand-worked cases.
"""
import numpy as np

NAMES = ('coff', 'outer', 'offset', 'rev', 'n_occ', 'n_inner', 'support', 'collapse_to', 'collapsed_reads')
DTYPES = {'coff': np.int64, 'outer': np.int32, 'offset': np.int32, 'rev': np.uint8, 'n_occ': np.int32,
          'n_inner': np.int32, 'support': np.int64, 'collapse_to': np.int32, 'collapsed_reads': np.int64}


def occurrences(A, B):
    """The (offset, direction) occurrences of row A in row B, ascending."""
    a, b = len(A), len(B)
    if a >= b:
        return []
    R = tuple(t ^ 1 for t in reversed(A))
    out = []
    for o in range(b - a + 1):
        window = B[o:o + a]
        if window == A:
            out.append((o, 0))
        if R != A and window == R:
            out.append((o, 1))
    return out


def containment(p):
    """The result as a dict of arrays (NAMES, DTYPES) for the path rows ``p`` (paths_ref.paths' dict)."""
    off, tok_off = np.asarray(p['off'], np.int64).tolist(), np.asarray(p['tok_off'], np.int64).tolist()
    n_rows = len(tok_off) - 1
    t = (np.asarray(p['locus'], np.int64) * 2 + np.asarray(p['rev'], np.int64)).tolist()
    rows = [tuple(t[a:b]) for a, b in zip(tok_off[:-1], tok_off[1:])]
    n_reads = np.asarray(p['n_reads'], np.int64).tolist()
    pairs = {}                                        # (inner, outer) -> occurrences
    for lo, hi in zip(off[:-1], off[1:]):
        for A in range(lo, hi):
            for B in range(lo, hi):
                occ = occurrences(rows[A], rows[B])
                if occ:
                    pairs[(A, B)] = occ
    order = sorted(pairs)
    coff = np.zeros(n_rows + 1, np.int64)
    for A, _ in order:
        coff[A + 1] += 1
    np.cumsum(coff, out=coff)
    n_inner, support = np.zeros(n_rows, np.int32), np.asarray(n_reads, np.int64).copy()
    for A, B in order:
        n_inner[B] += 1
        support[B] += n_reads[A]
    contained = {A for A, _ in order}
    collapse_to = np.arange(n_rows, dtype=np.int32)
    for A in sorted(contained):
        best = [B for (X, B) in order if X == A and B not in contained]
        assert best, 'containment is transitive: a contained row lies in a maximal one'
        collapse_to[A] = min(best, key=lambda B: (-int(support[B]), B))
    collapsed = np.zeros(n_rows, np.int64)
    for A in range(n_rows):
        collapsed[collapse_to[A]] += n_reads[A]
    first = [min(pairs[k]) for k in order]
    return {'coff': coff, 'outer': np.asarray([B for _, B in order], np.int32),
            'offset': np.asarray([o for o, _ in first], np.int32), 'rev': np.asarray([d for _, d in first], np.uint8),
            'n_occ': np.asarray([len(pairs[k]) for k in order], np.int32), 'n_inner': n_inner, 'support': support,
            'collapse_to': collapse_to, 'collapsed_reads': collapsed}


def paths_of_rows(clusters):
    """A paths_ref-shaped dict from hand-written rows: ``clusters`` is a list of clusters, each a list of (tokens
    tuple, n_reads); the rows of a cluster are put in ascending order, as fslr_cluster_paths leaves them."""
    off, tok_off, n_reads, toks = [0], [0], [], []
    for rows in clusters:
        for tk, k in sorted(rows):
            toks.extend(tk), n_reads.append(k), tok_off.append(len(toks))
        off.append(len(n_reads))
    toks = np.asarray(toks, np.int64)
    return {'off': np.asarray(off, np.int64), 'tok_off': np.asarray(tok_off, np.int64), 'n_reads': np.asarray(n_reads, np.int32),
            'locus': (toks >> 1).astype(np.int32), 'rev': (toks & 1).astype(np.uint8)}
