"""The plain statement of the cluster paths (include/fslr_hip.h fslr_cluster_paths), on the host, on top of
tests/loci_ref.py and junctions_ref.locus_row.

Every clustered read, one-interval reads included, is a chain: its intervals ordered by (query key, CSR position).
An interval gives the token t = locus_row * 2 + rev.  F is the chain's tuple of tokens, B = the tuple reversed with
every low bit flipped (the same molecule read from the other strand); the read's path is min(F, B) and flipped =
B < F.  Python's tuple order is the specified one: lexicographic, a proper prefix before its extensions.  A row per
distinct path in ascending order (sorted(set(...))): n_reads, first_read (the smallest rank), its tokens behind
tok_off; off[n_clusters + 1] gives each cluster's rows; path_of_read and flipped are per read.
tests/test_paths_ref.py pins it to hand-worked cases.
"""
import numpy as np

import junctions_ref
import loci_ref

NAMES = ('off', 'tok_off', 'n_reads', 'first_read', 'locus', 'rev', 'path_of_read', 'flipped')
DTYPES = {'off': np.int64, 'tok_off': np.int64, 'n_reads': np.int32, 'first_read': np.int32, 'locus': np.int32,
          'rev': np.uint8, 'path_of_read': np.int32, 'flipped': np.uint8}


def paths(read_off, iv_chrom, iv_start, iv_end, cid, n_clusters, qkey, rev=None, loci=None):
    """The result as a dict of arrays (NAMES, DTYPES).  ``qkey`` and ``rev`` (None: all 0) are per CSR interval;
    ``loci`` are loci_ref.loci's rows (made here when None)."""
    read_off = np.asarray(read_off, np.int64)
    n = read_off.shape[0] - 1
    if loci is None:
        loci = loci_ref.loci(read_off, iv_chrom, iv_start, iv_end, cid, n_clusters)
    path, flipped = {}, np.zeros(n, np.uint8)
    for r in range(n):
        c = int(cid[r])
        if c < 0:
            continue
        ks = sorted(range(int(read_off[r]), int(read_off[r + 1])), key=lambda k: (int(qkey[k]), k))
        F = tuple(junctions_ref.locus_row(loci, c, int(iv_chrom[k]), int(iv_start[k])) * 2 +
                  (int(bool(rev[k])) if rev is not None else 0) for k in ks)
        B = tuple(t ^ 1 for t in reversed(F))
        path[r] = min(F, B)
        flipped[r] = B < F
    rows = sorted(set(path.values()))
    row_of = {p: i for i, p in enumerate(rows)}
    path_of_read = np.full(n, -1, np.int32)
    n_reads, first_read = np.zeros(len(rows), np.int32), np.full(len(rows), n, np.int32)
    for r in sorted(path):
        i = row_of[path[r]]
        path_of_read[r] = i
        n_reads[i] += 1
        first_read[i] = min(first_read[i], r)
    cluster_of_locus = np.repeat(np.arange(n_clusters), np.diff(loci['off']))
    per_cluster = np.zeros(n_clusters, np.int64)
    for p in rows:
        per_cluster[cluster_of_locus[p[0] >> 1]] += 1
    off, tok_off = np.zeros(n_clusters + 1, np.int64), np.zeros(len(rows) + 1, np.int64)
    np.cumsum(per_cluster, out=off[1:])
    np.cumsum([len(p) for p in rows], out=tok_off[1:])
    toks = [t for p in rows for t in p]
    return {'off': off, 'tok_off': tok_off, 'n_reads': n_reads, 'first_read': first_read,
            'locus': np.asarray([t >> 1 for t in toks], np.int32), 'rev': np.asarray([t & 1 for t in toks], np.uint8),
            'path_of_read': path_of_read, 'flipped': flipped}


def paths_of_csr(csr, labels, qkey, rev=None):
    """paths() for a prep.CSR (real reads) and min-rank labels."""
    cid, nc = loci_ref.cids_of_labels(labels)
    return paths(csr.read_off, csr.iv_chrom, csr.iv_start, csr.iv_end, cid, nc, qkey, rev)


def rows_of(res):
    """The rows as a list of (tokens tuple, n_reads, first_read)."""
    t = (res['locus'].astype(np.int64) * 2 + res['rev']).tolist()
    o = res['tok_off'].tolist()
    return [(tuple(t[a:b]), int(k), int(f)) for a, b, k, f in zip(o[:-1], o[1:], res['n_reads'], res['first_read'])]
