"""The plain statement of the cluster junctions (include/fslr_hip.h fslr_cluster_junctions), on the host, on
top of tests/loci_ref.py.

Every clustered read of two or more intervals is a chain: its intervals ordered by (query key, CSR position).
Each consecutive pair (x, y) is one observation.  An interval lies in the locus row of its read's cluster with its
chromosome and start <= iv.start <= end.  The chain leaves x at its right end (side 1, breakpoint x.end) when
rev[x] == 0, else at its left end (side 0, x.start); it enters y at its left end (side 0, y.start) when
rev[y] == 0, else at its right end (side 1, y.end).  An end is e = locus_row * 2 + side; the observation is the
unordered pair, smaller end first with its breakpoint (on equal ends the smaller breakpoint first).  A row per
distinct (ea, eb) in ascending order: locus_a, side_a, locus_b, side_b, n_obs, n_reads (a Python set) and the
extrema of the two breakpoints; off[n_clusters + 1] gives each cluster's rows.  tests/test_junctions_ref.py pins
it to hand-worked cases.
"""
import numpy as np

import loci_ref

COLUMNS = ('locus_a', 'side_a', 'locus_b', 'side_b', 'n_obs', 'n_reads', 'bp_a_min', 'bp_a_max', 'bp_b_min', 'bp_b_max')
DTYPES = dict.fromkeys(COLUMNS, np.int32) | {'side_a': np.uint8, 'side_b': np.uint8}


def locus_row(loci, c, chrom, start):
    """The one row of cluster c that holds an interval of ``chrom`` starting at ``start``."""
    hits = [k for k in range(int(loci['off'][c]), int(loci['off'][c + 1]))
            if loci['chrom'][k] == chrom and loci['start'][k] <= start <= loci['end'][k]]
    assert len(hits) == 1, (c, chrom, start, hits)
    return hits[0]


def junctions(read_off, iv_chrom, iv_start, iv_end, cid, n_clusters, qkey, rev=None, loci=None):
    """The rows as a dict of arrays: ``off`` int64[n_clusters + 1] and COLUMNS.  ``qkey`` and ``rev`` (None: all
    0) are per CSR interval; ``loci`` are loci_ref.loci's rows (made here when None)."""
    read_off = np.asarray(read_off, np.int64)
    if loci is None:
        loci = loci_ref.loci(read_off, iv_chrom, iv_start, iv_end, cid, n_clusters)
    rows = {}                                      # (ea, eb) -> [n_obs, reads, a_min, a_max, b_min, b_max]
    for r in range(read_off.shape[0] - 1):
        c = int(cid[r])
        ks = list(range(int(read_off[r]), int(read_off[r + 1])))
        if c < 0 or len(ks) < 2:
            continue
        ks.sort(key=lambda k: (int(qkey[k]), k))
        for x, y in zip(ks[:-1], ks[1:]):
            rx = bool(rev[x]) if rev is not None else False
            ry = bool(rev[y]) if rev is not None else False
            lx = locus_row(loci, c, int(iv_chrom[x]), int(iv_start[x]))
            ly = locus_row(loci, c, int(iv_chrom[y]), int(iv_start[y]))
            a = (lx * 2 + (0 if rx else 1), int(iv_start[x]) if rx else int(iv_end[x]))
            b = (ly * 2 + (1 if ry else 0), int(iv_end[y]) if ry else int(iv_start[y]))
            if b < a:                              # the smaller end first; on equal ends the smaller breakpoint
                a, b = b, a
            row = rows.setdefault((a[0], b[0]), [0, set(), a[1], a[1], b[1], b[1]])
            row[0] += 1
            row[1].add(r)
            row[2], row[3] = min(row[2], a[1]), max(row[3], a[1])
            row[4], row[5] = min(row[4], b[1]), max(row[5], b[1])
    keys = sorted(rows)
    per_cluster = np.zeros(n_clusters, np.int64)
    cluster_of_locus = np.repeat(np.arange(n_clusters), np.diff(loci['off']))
    for ea, _ in keys:
        per_cluster[cluster_of_locus[ea >> 1]] += 1
    off = np.zeros(n_clusters + 1, np.int64)
    np.cumsum(per_cluster, out=off[1:])
    vals = {'locus_a': [ea >> 1 for ea, _ in keys], 'side_a': [ea & 1 for ea, _ in keys],
            'locus_b': [eb >> 1 for _, eb in keys], 'side_b': [eb & 1 for _, eb in keys],
            'n_obs': [rows[k][0] for k in keys], 'n_reads': [len(rows[k][1]) for k in keys],
            'bp_a_min': [rows[k][2] for k in keys], 'bp_a_max': [rows[k][3] for k in keys],
            'bp_b_min': [rows[k][4] for k in keys], 'bp_b_max': [rows[k][5] for k in keys]}
    out = {'off': off}
    for name in COLUMNS:
        out[name] = np.asarray(vals[name], DTYPES[name])
    return out


def junctions_of_csr(csr, labels, qkey, rev=None):
    """junctions() for a prep.CSR (real reads) and min-rank labels."""
    cid, nc = loci_ref.cids_of_labels(labels)
    return junctions(csr.read_off, csr.iv_chrom, csr.iv_start, csr.iv_end, cid, nc, qkey, rev)


def reverse_complement(read_off, qkey, rev, reads):
    """(qkey, rev) with the chains of ``reads`` reversed and their rev bits flipped: the same molecules read from
    the other strand."""
    qkey, rev = np.array(qkey, np.int64), np.array(rev, np.uint8)
    for r in reads:
        s = slice(int(read_off[r]), int(read_off[r + 1]))
        qkey[s] = -qkey[s] - 1                    # reverses the order; equal keys stay equal
        rev[s] ^= 1
    return qkey, rev
