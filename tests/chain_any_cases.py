"""Hand-built inputs for the tests of fslr_cluster_junctions_any / fslr_cluster_paths_any: a handful of reads of chosen
interval counts on a few loci, and query keys made per position in the real CSR's lists."""
import numpy as np

import search_ref as sr
from fslr_amd import cluster

GAP = 100000                   # loci are GAP apart: the intervals of one never reach the next


def index_of_lens(ctx, lens, n_loci=6, seed=0):
    """Reads of the given interval counts (the ranks follow the reads' first starts: find a read by its length, or
    through ``csr.read_qcode``, which holds its place in ``lens``).  Every interval lies in one of ``n_loci``
    loci (locus a: chromosome a % 2, starts in [GAP a, GAP a + 5000), ends beyond every start of the locus, so all
    the intervals of a locus merge), chosen at random per interval."""
    rng = np.random.default_rng(seed)
    chrom, start, end, read = [], [], [], []
    for k, n in enumerate(lens):
        for a in rng.integers(0, n_loci, n).tolist():
            chrom.append(a % 2), read.append(k)
            start.append(GAP * a + int(rng.integers(0, 5000)))
            end.append(GAP * a + 6000 + int(rng.integers(0, 3000)))
    return index_of(ctx, chrom, start, end, read, lens)


def index_of(ctx, chrom, start, end, read, lens):
    idx = cluster.build_interval_trees(sr.make_data(chrom, start, end, qcode=read), ctx=ctx)
    assert np.diff(idx.csr.read_off).tolist() == [lens[k] for k in np.asarray(idx.csr.read_qcode).tolist()]
    assert (idx.long is not None) == (max(lens) > 64)
    return idx


def index_of_walks(ctx, walks):
    """Reads that walk given loci: ``walks[k]`` is a list of (locus, rev); the t-th piece starts at GAP locus + 8 t
    + k % 8, so within a locus the CSR order is the walk's order.  Returns the index and (qkey, rev) per CSR interval
    with qkey = the piece's place in its walk."""
    chrom, start, end, read, info = [], [], [], [], {}
    for k, w in enumerate(walks):
        for t, (a, v) in enumerate(w):
            s = GAP * a + 8 * t + k % 8
            chrom.append(0), start.append(s), end.append(GAP * a + 50000 + t), read.append(k)
            info[(k, s)] = (t, int(v))
    idx = index_of(ctx, chrom, start, end, read, [len(w) for w in walks])
    csr = idx.csr
    walk = np.repeat(np.asarray(csr.read_qcode), np.diff(csr.read_off))           # the rank's place in ``walks``
    kv = np.asarray([info[(int(k), int(s))] for k, s in zip(walk, np.asarray(csr.iv_start))], np.int64)
    return idx, kv[:, 0].astype(np.int32), kv[:, 1].astype(np.uint8)


def place(csr):
    """Each CSR interval's position in its read's list."""
    off = np.asarray(csr.read_off, np.int64)
    return np.arange(csr.n_intervals) - np.repeat(off[:-1], np.diff(off))


KEY_MODES = ('ascending', 'descending', 'shuffled', 'equal', 'seam_equal', 'seam_extremes')


def keys_of(csr, mode):
    """Query keys per CSR interval from the position j in the list.  seam_equal: positions 63 and 64, the last of the
    first chunk and the first of the second, share a key, so the list order decides across the seam.  seam_extremes:
    the smallest key stands at position 64 and the largest at position 0."""
    j = place(csr)
    if mode == 'ascending':
        return j.astype(np.int32)
    if mode == 'descending':
        return (-j).astype(np.int32)
    if mode == 'shuffled':
        return np.random.default_rng(17).permutation(csr.n_intervals).astype(np.int32)
    if mode == 'equal':
        return np.full(csr.n_intervals, -3, np.int32)
    if mode == 'seam_equal':
        return np.where(j == 64, 63, j).astype(np.int32)
    assert mode == 'seam_extremes'
    k = (j * 7919) % 4099                                             # a fixed scramble, below the extremes
    return np.where(j == 64, -(1 << 31), np.where(j == 0, (1 << 31) - 1, k)).astype(np.int32)


def rank_of_walk(csr, k):
    """The rank of the k-th read given to index_of_lens / index_of_walks."""
    return int(np.flatnonzero(np.asarray(csr.read_qcode) == k)[0])


def one_cluster(csr, alone=()):
    """Min-rank labels: every read in one cluster but those given in ``alone`` (places in the list the index was
    made from)."""
    lab = np.arange(csr.n_reads, dtype=np.int32)
    members = np.flatnonzero(~np.isin(np.asarray(csr.read_qcode), list(alone)))
    lab[members] = members.min()
    return lab


def groups_of(n, size):
    """Min-rank labels: clusters of ``size`` consecutive ranks (a last one of a single read stays alone)."""
    return (np.arange(n, dtype=np.int32) // size) * size
