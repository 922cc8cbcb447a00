"""The plain statement of the cluster loci (include/fslr_hip.h fslr_cluster_loci), on the host.

For every cluster (dense id of the cluster table, components of two or more reads) take every interval of its
member reads, group them by chromosome, walk each group in ascending start: an interval opens a new locus iff
it is the group's first or its start is greater than the largest end seen so far in the group (end-inclusive:
start == that end merges, start == that end + 1 does not).  A row per locus - chrom, start (the first
interval's), end (the largest), n_intervals, n_reads (distinct reads, a Python set) - ordered by (cluster,
chrom, start); off[n_clusters + 1] gives each cluster's rows.  tests/test_loci_ref.py pins it to hand-worked
cases and to a second statement by per-position coverage.
"""
import numpy as np

COLUMNS = ('chrom', 'start', 'end', 'n_intervals', 'n_reads')


def cids_of_labels(labels):
    """(cid per read, n_clusters) of min-rank labels: the components of two or more reads numbered by
    ascending smallest rank, -1 for a read alone (the cluster table's dense ids)."""
    labels = np.asarray(labels, np.int64)
    n = labels.shape[0]
    size = np.bincount(labels, minlength=n)
    roots = np.flatnonzero(size >= 2)
    dense = np.full(n, -1, np.int64)
    dense[roots] = np.arange(roots.size)
    return (dense[labels] if n else dense), int(roots.size)


def loci(read_off, iv_chrom, iv_start, iv_end, cid, n_clusters):
    """The rows as a dict of arrays: ``off`` int64[n_clusters + 1] and COLUMNS as int32.  ``read_off`` is the
    CSR of the real reads; ``cid[r]`` the cluster of read r or -1."""
    read_off = np.asarray(read_off, np.int64)
    groups = {}                                   # (cluster, chrom) -> [(start, end, read)]
    for r in range(read_off.shape[0] - 1):
        c = int(cid[r])
        if c < 0:
            continue
        for k in range(int(read_off[r]), int(read_off[r + 1])):
            groups.setdefault((c, int(iv_chrom[k])), []).append((int(iv_start[k]), int(iv_end[k]), r))
    rows, per_cluster = [], np.zeros(n_clusters, np.int64)
    for (c, ch) in sorted(groups):
        cur = None
        for s, e, r in sorted(groups[(c, ch)]):
            if cur is None or s > cur[2]:
                if cur is not None:
                    rows.append(cur)
                cur = [ch, s, e, 0, set(), c]
                per_cluster[c] += 1
            cur[2] = max(cur[2], e)
            cur[3] += 1
            cur[4].add(r)
        rows.append(cur)
    off = np.zeros(n_clusters + 1, np.int64)
    np.cumsum(per_cluster, out=off[1:])
    out = {'off': off}
    for k, name in enumerate(COLUMNS):
        out[name] = np.asarray([len(x[k]) if name == 'n_reads' else x[k] for x in rows], np.int32)
    return out


def loci_of_csr(csr, labels):
    """loci() for a prep.CSR (real reads) and min-rank labels."""
    cid, nc = cids_of_labels(labels)
    return loci(csr.read_off, csr.iv_chrom, csr.iv_start, csr.iv_end, cid, nc)


def bed_text(rows, chrom_names):
    """The rows as the CLI writes them: tab-separated, header ``cluster chrom start end n_intervals n_reads``;
    ``chrom_names[d]`` names dense chromosome d."""
    lines = ['\t'.join(('cluster',) + ('chrom', 'start', 'end', 'n_intervals', 'n_reads'))]
    cl = np.repeat(np.arange(rows['off'].shape[0] - 1), np.diff(rows['off']))
    for k in range(cl.shape[0]):
        lines.append('\t'.join([str(int(cl[k])), str(chrom_names[int(rows['chrom'][k])])] +
                               [str(int(rows[c][k])) for c in COLUMNS[1:]]))
    return '\n'.join(lines) + '\n'
