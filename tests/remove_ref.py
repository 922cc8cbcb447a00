"""What fslr_remove_reads must leave behind, stated in numpy: the kept reads with the gaps closed in rank, in
CSR order and in the start-sorted `data` list, the dense chromosome ids and n_chroms as they were: the CSR a
fresh fslr_set_reads of the survivors would take."""
import numpy as np

from fslr_amd.prep import CSR


def rank_map(keep):
    """Old rank -> new rank (#{kept reads of lower rank}), -1 for a removed read."""
    keep = np.asarray(keep, bool)
    return np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)


def kept_rows(csr, keep):
    """Per position of the `data` list: does its element stay (its read is kept)."""
    keep_iv = np.repeat(np.asarray(keep, bool), np.diff(np.asarray(csr.read_off, np.int64)))
    rows = np.empty(csr.n_intervals, bool)
    rows[np.asarray(csr.data_pos, np.int64)] = keep_iv
    return rows


def remove_csr(csr, keep):
    """``(compacted CSR, its data_pos, old rank -> new rank)`` for a mask over the read ranks (True = the read
    stays).  A kept interval at data position d moves to #{kept elements before d}; read r's intervals sit at
    CSR offset = the sum of the kept lower reads' lengths, in their old order.  Keeping nothing is refused
    (ValueError), keeping everything returns the CSR's own columns."""
    keep = np.asarray(keep, bool)
    if keep.shape != (csr.n_reads,):
        raise ValueError('one mask entry per read')
    if not keep.any():
        raise ValueError('would leave no reads')
    L = np.diff(np.asarray(csr.read_off, np.int64))
    keep_iv = np.repeat(keep, L)
    rows = kept_rows(csr, keep)
    newpos = np.cumsum(rows) - rows                                 # exclusive count of kept elements
    off = np.zeros(int(keep.sum()) + 1, np.int64)
    np.cumsum(L[keep], out=off[1:])
    dp = newpos[np.asarray(csr.data_pos, np.int64)[keep_iv]]
    out = CSR(read_off=off.astype(np.int32), read_qlen2=csr.read_qlen2[keep], read_nal=csr.read_nal[keep],
              iv_chrom=csr.iv_chrom[keep_iv], iv_start=csr.iv_start[keep_iv], iv_end=csr.iv_end[keep_iv],
              iv_aln=csr.iv_aln[keep_iv], n_chroms=csr.n_chroms, read_qcode=np.asarray(csr.read_qcode)[keep],
              data_pos=dp, nal_varies=csr.nal_varies, start_sorted=True)
    return out, dp, rank_map(keep)
