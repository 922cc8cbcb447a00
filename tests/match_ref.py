"""The expected result of matching new reads against a resident index (fslr_match_reads), on the CPU, from
what the other tests already trust: the candidates and their order from search_ref.brute_force (the
fslr_search order contract) reduced to first visits, I / U and calculate_overlap's ZeroDivisionError from
oracle.jaccard_lists, the length gate from oracle.lengths_differ, the flag byte as fslr_score_pairs
defines it.  Also the small builders the match tests share."""
import numpy as np

import search_ref as sr
from fslr_amd import _lib
from fslr_amd._lib import SCORE_EDGE, SCORE_GATE, SCORE_ZD_GATE, SCORE_ZD_OVERLAP
from fslr_amd.prep import IntervalData, fold_overlap_threshold
from oracle import oracle as O


def resident_data(reads, qlen2, nal, shuffle_seed=None) -> IntervalData:
    """The `data` list of ``reads`` (per read a list of (chrom, start, end, aln_size)) in non-decreasing
    start order; ties of equal start keep the given order or a seeded shuffle of it.  Read k is 'r<k>'."""
    code = np.repeat(np.arange(len(reads)), [len(r) for r in reads])
    flat = np.array([x for r in reads for x in r], np.int64).reshape(-1, 4)
    n = flat.shape[0]
    first = np.arange(n) if shuffle_seed is None else np.random.default_rng(shuffle_seed).permutation(n)
    o = first[np.argsort(flat[first, 1], kind='stable')]
    q2, na = np.asarray(qlen2, np.int64), np.asarray(nal, np.int64)
    return IntervalData(chrom=flat[o, 0], start=flat[o, 1], end=flat[o, 2], aln_size=flat[o, 3], qcode=code[o],
                        qnames=np.asarray([f'r{k}' for k in range(len(reads))], dtype=object),
                        n_alignments=na[code[o]], qlen2=q2[code[o]], middle=(flat[o, 1] + flat[o, 2]) // 2,
                        index=np.arange(n, dtype=np.int64))


class Queries:
    """Query reads as the C ABI takes them: per read a list of (chrom, start, end, aln_size) in loop order,
    ``chrom`` in the resident data's own values."""

    def __init__(self, reads, qlen2, nal, exclude=None):
        self.reads = [list(r) for r in reads]
        self.qlen2, self.nal = np.asarray(qlen2, np.int32), np.asarray(nal, np.int32)
        self.exclude = None if exclude is None else np.asarray(exclude, np.int32)
        self.off = np.zeros(len(reads) + 1, np.int32)
        self.off[1:] = np.cumsum([len(r) for r in reads])
        self.flat = np.array([x for r in reads for x in r], np.int64).reshape(-1, 4)

    def __len__(self):
        return len(self.reads)

    def dense_chrom(self, data):
        """The CSR's dense ids (ascending over the chromosomes present); -1 for one the data lacks."""
        keys = np.unique(np.asarray(data.chrom))
        at = np.minimum(np.searchsorted(keys, self.flat[:, 0]), max(keys.size - 1, 0))
        return np.where(keys[at] == self.flat[:, 0], at, -1).astype(np.int32) if keys.size else \
            np.full(self.flat.shape[0], -1, np.int32)

    def run(self, ctx, data, pct, qd, nd, pt, emit_mask, exclude='own'):
        """fslr_match_reads + fslr_match_rows through the binding: (offsets, partner, I, U, flags, counts, best)."""
        ex = self.exclude if isinstance(exclude, str) else exclude
        off, counts, best = ctx.match_reads(self.off, self.qlen2, self.nal, self.dense_chrom(data), self.flat[:, 1],
                                            self.flat[:, 2], fold_overlap_threshold(self.flat[:, 3], pct), 1 - qd,
                                            1 - nd, pt, emit_mask, ex)
        return (off, *ctx.match_rows(), counts, best)


def flag_byte(I, U, zd, q1, q2, n1, n2, qd, nd, pt):
    """The flag byte the reference's predicates give the pair (fslr_hip.h FSLR_SCORE_*)."""
    try:
        flags = 0 if O.lengths_differ(q1, q2, n1, n2, qd, nd) else SCORE_GATE
    except ZeroDivisionError:
        flags = SCORE_ZD_GATE
    if zd:
        return flags | SCORE_ZD_OVERLAP
    if flags & SCORE_GATE and I > 0 and pt.reshape(-1, _lib.PASS_STRIDE)[I - 1, U - 1]:
        flags |= SCORE_EDGE
    return flags


def candidates(data, csr, queries):
    """Per query read its hit count and the distinct resident ranks its loop meets, in first-visit order
    (the excluded rank included: the caller drops it)."""
    read_of_pos = np.empty(len(data), np.int64)
    read_of_pos[np.asarray(csr.data_pos, np.int64)] = np.repeat(np.arange(csr.n_reads), np.diff(csr.read_off))
    f = queries.flat
    off, pos = sr.brute_force(data.chrom, data.start, data.end, f[:, 0], f[:, 1], f[:, 2])
    out, hits = [], []
    for q in range(len(queries)):
        p = read_of_pos[pos[off[queries.off[q]]:off[queries.off[q + 1]]]]
        _, first = np.unique(p, return_index=True)
        out.append(p[np.sort(first)])
        hits.append(int(p.size))
    return out, hits


def match_ref(data, csr, queries, pct, qd, nd, pt, emit_mask):
    """``(offsets, partner, I, U, flags, counts, best)`` as fslr_match_reads + fslr_match_rows return them."""
    lists = []
    dp = np.asarray(csr.data_pos, np.int64)
    for r in range(csr.n_reads):
        k = dp[csr.read_off[r]:csr.read_off[r + 1]]
        lists.append(list(zip(data.chrom[k].tolist(), data.start[k].tolist(), data.end[k].tolist(),
                              data.aln_size[k].tolist())))
    cands, _ = candidates(data, csr, queries)
    rows, off, counts, best = [], [0], [], []
    for q, cs in enumerate(cands):
        ex = -1 if queries.exclude is None else int(queries.exclude[q])
        n_c = n_g = n_e = 0
        top = (-1, 0, 1)
        for p in cs.tolist():
            if p == ex:
                continue
            try:
                I, U, zd = (*O.jaccard_lists(queries.reads[q], lists[p], pct), False)
            except ZeroDivisionError:
                I, U, zd = 0, 0, True
            fl = flag_byte(I, U, zd, int(queries.qlen2[q]), int(csr.read_qlen2[p]), int(queries.nal[q]),
                           int(csr.read_nal[p]), qd, nd, pt)
            n_c += 1
            n_g += bool(fl & SCORE_GATE)
            if fl & SCORE_EDGE:
                n_e += 1
                if top[0] < 0 or I * top[2] > top[1] * U:
                    top = (p, I, U)
            if emit_mask == 0 or fl & emit_mask:
                rows.append((p, I, U, fl))
        off.append(len(rows))
        counts.append((n_c, n_g, n_e))
        best.append(top[0])
    r = np.array(rows, np.int64).reshape(-1, 4)
    return (np.asarray(off, np.int64), r[:, 0].astype(np.int32), r[:, 1].astype(np.int32), r[:, 2].astype(np.int32),
            r[:, 3].astype(np.uint8), np.array(counts, np.int32).reshape(-1, 3), np.asarray(best, np.int32))
