"""Inputs with contained paths for the tests of fslr_cluster_path_containment: a golden fixture whose clustered reads
lose a piece at one end, as a truncated read does, under the fixture's own clusters."""
import numpy as np

from test_gpu_junctions import bed_inputs
from test_gpu_loci import fixture_membership


def truncated_fixture(name):
    """The fixture's data list without one end piece of every second clustered read of two or more intervals: the
    piece with the smallest query start and the one with the largest, in turn.  Returns ``(data, qstart, rev,
    cid_of_code)``: the columns are aligned with the shortened data list (its ``index`` still names the rows of the
    fixture's .mappings.bed); ``cid_of_code`` is the cluster of the fixture's expected output per qname code (-1: a
    read alone), so that with ``labels_for`` a truncated read stays with the full-length reads of its cluster."""
    data, csr, cid, nc, kw = fixture_membership(name)
    qstart, _, rev = bed_inputs(name, data)
    code_of_rank = np.asarray(csr.read_qcode)
    cid_of_code = np.full(int(code_of_rank.max()) + 1, -1, np.int64)
    cid_of_code[code_of_rank] = cid
    qcode = np.asarray(data.qcode)
    keep = np.ones(qcode.size, bool)
    lens = np.diff(np.asarray(csr.read_off, np.int64))
    for i, r in enumerate(np.flatnonzero((cid >= 0) & (lens >= 2)).tolist()[::2]):
        at = np.flatnonzero(qcode == code_of_rank[r])
        keep[at[np.argmin(qstart[at]) if i % 2 == 0 else np.argmax(qstart[at])]] = False
    return data.select(keep), qstart[keep], rev[keep], cid_of_code


def labels_for(csr, cid_of_code):
    """Min-rank labels of ``csr``'s reads from the cluster of each qname code; a cluster left with one read stays
    alone."""
    c = cid_of_code[np.asarray(csr.read_qcode)]
    lab = np.arange(csr.n_reads, dtype=np.int32)
    for k in np.unique(c[c >= 0]).tolist():
        m = np.flatnonzero(c == k)
        lab[m] = m.min()
    return lab
