"""What fslr_append_reads must leave behind, stated in numpy: where every element of the resident and of
the new start-sorted `data` list lands in their stable merge (the resident element first on equal starts),
and the concatenated CSR a fresh fslr_set_reads of the union would take."""
import numpy as np

from fslr_amd.prep import CSR


def merged_positions(res_starts, new_starts):
    """``(pos_res, pos_new)``: a resident element at data position d with start s moves to
    d + #{new starts < s}; a new element at its own position e with start t lands at
    e + #{resident starts <= t}.  Both inputs are in non-decreasing order."""
    a, b = np.asarray(res_starts, np.int64), np.asarray(new_starts, np.int64)
    assert (np.diff(a) >= 0).all() and (np.diff(b) >= 0).all()
    pos_res = np.arange(a.size, dtype=np.int64) + np.searchsorted(b, a, side='left')
    pos_new = np.arange(b.size, dtype=np.int64) + np.searchsorted(a, b, side='right')
    return pos_res, pos_new


def data_starts(csr):
    """The starts of a CSR's intervals in its data order."""
    s = np.empty(csr.n_intervals, np.int64)
    s[np.asarray(csr.data_pos, np.int64)] = csr.iv_start
    return s


def concat_csr(res, new, n_chroms=None):
    """The CSR of the union: the resident reads' rows, then the new reads' (``new.iv_chrom`` in the resident
    dense ids), with the merged data positions."""
    pos_res, pos_new = merged_positions(data_starts(res), data_starts(new))
    cat = lambda f: np.concatenate([getattr(res, f), getattr(new, f)])
    return CSR(read_off=np.concatenate([res.read_off, res.n_intervals + np.asarray(new.read_off)[1:]]).astype(np.int32),
               read_qlen2=cat('read_qlen2'), read_nal=cat('read_nal'), iv_chrom=cat('iv_chrom'), iv_start=cat('iv_start'),
               iv_end=cat('iv_end'), iv_aln=cat('iv_aln'), n_chroms=int(n_chroms or max(res.n_chroms, new.n_chroms)),
               read_qcode=np.concatenate([res.read_qcode, np.asarray(new.read_qcode) + (int(np.max(res.read_qcode, initial=-1)) + 1)]),
               data_pos=np.concatenate([pos_res[np.asarray(res.data_pos, np.int64)],
                                        pos_new[np.asarray(new.data_pos, np.int64)]]),
               nal_varies=bool(res.nal_varies or new.nal_varies), start_sorted=True)
