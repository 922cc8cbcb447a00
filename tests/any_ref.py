"""Reference and directed inputs for pair scoring over reads of any length (fslr_score_pairs_any: lists of
up to 4096 intervals, I up to 4096, U up to 8191).  Test infrastructure only; not a test module.

The reference: I, U and calculate_overlap's ZeroDivisionError from the C oracle's overall_jaccard_similarity
(oracle.jaccard_lists, lists of any length), the gate from oracle.lengths_differ, EDGE from Python floats,
``I / U >= cut[min(I, len(cut)) - 1]`` (cluster.py:216-219).  match_ref.flag_byte indexes the pass table
and cannot serve I > 64.

The inputs are plain lists: a read is a list of (chrom, start, end, aln_size) in list order.
"""
import numpy as np

from fslr_amd._lib import SCORE_EDGE, SCORE_GATE, SCORE_ZD_GATE, SCORE_ZD_OVERLAP
from oracle import oracle as O

QLEN2, NAL = 1000, 4
QLEN_DIFF, NAL_DIFF = 0.04, 0.25
CUTS = [1, 1, 0.66, 0.66, 0.66, 0.5]
SEAM_LENGTHS = (1, 63, 64, 65, 127, 128, 129, 4095, 4096)


def fit(l1, l2, overlap):
    """(I, U, zd) of overall_jaccard_similarity(l1, l2); where calculate_overlap raises: (0, 0, True)."""
    try:
        return (*O.jaccard_lists(l1, l2, overlap), False)
    except ZeroDivisionError:
        return 0, 0, True


def flag_byte(I, U, zd, q1, q2, n1, n2, cuts, qlen_diff=QLEN_DIFF, diff=NAL_DIFF):
    """The FSLR_SCORE_* bits of a pair with first-fit result (I, U, zd) and the two reads' qlen2 / n_alignments."""
    try:
        flags = 0 if O.lengths_differ(q1, q2, n1, n2, qlen_diff, diff) else SCORE_GATE
    except ZeroDivisionError:
        flags = SCORE_ZD_GATE
    if zd:
        return flags | SCORE_ZD_OVERLAP
    cut = [float(c) for c in cuts]
    if flags & SCORE_GATE and I > 0 and I / U >= cut[min(I, len(cut)) - 1]:
        flags |= SCORE_EDGE
    return flags


class Pool:
    """Reads gathered for one upload, the pairs asked of them, and the reference's answers (each distinct
    ordered pair is scored once per overlap cutoff)."""

    def __init__(self, overlap):
        self.overlap = overlap
        self.reads, self.qlen2, self.nal = [], [], []
        self._fit = {}

    def add(self, read, qlen2=QLEN2, nal=NAL):
        self.reads.append(list(read))
        self.qlen2.append(qlen2)
        self.nal.append(nal)
        return len(self.reads) - 1

    def csr(self):
        """What Context.load_csr_any / load_csr take: the reads in the pool's order, no data order."""
        from types import SimpleNamespace
        off = np.zeros(len(self.reads) + 1, np.int64)
        off[1:] = np.cumsum([len(r) for r in self.reads])
        flat = np.array([x for r in self.reads for x in r], np.int64).reshape(-1, 4)
        return SimpleNamespace(read_off=off.astype(np.int32), read_qlen2=np.asarray(self.qlen2, np.int32),
                               read_nal=np.asarray(self.nal, np.int32), iv_chrom=flat[:, 0].astype(np.int32),
                               iv_start=flat[:, 1].astype(np.int32), iv_end=flat[:, 2].astype(np.int32),
                               iv_aln=flat[:, 3], n_chroms=int(flat[:, 0].max()) + 1, start_sorted=False,
                               n_reads=len(self.reads), n_intervals=int(off[-1]))

    def max_len(self):
        return max(len(r) for r in self.reads)

    def expect(self, a, b, cuts, qlen_diff=QLEN_DIFF, diff=NAL_DIFF):
        """(I, U, flags) arrays for the ordered pairs (a[k], b[k]), every pair."""
        I, U, F = [], [], []
        for x, y in zip(a, b):
            x, y = int(x), int(y)
            if (x, y) not in self._fit:
                self._fit[(x, y)] = fit(self.reads[x], self.reads[y], self.overlap)
            i, u, zd = self._fit[(x, y)]
            I.append(i)
            U.append(u)
            F.append(flag_byte(i, u, zd, self.qlen2[x], self.qlen2[y], self.nal[x], self.nal[y], cuts, qlen_diff, diff))
        return np.asarray(I, np.int32), np.asarray(U, np.int32), np.asarray(F, np.uint8)


# ---------------------------------------------------------------------------------- builders
X = (1, 1000, 2000, 1000)                     # the interval every directed match is made of
Z = (1, 1000, 2000, 0)                        # the same with aln_size == 0: calculate_overlap divides by it


def diag(n, first=0):
    """Interval k at (first + k) * 10_000 on chromosome 1: diag(a) x diag(b) matches cell (k, k) alone."""
    return [(1, 10_000 * (first + k), 10_000 * (first + k) + 1000, 1000) for k in range(n)]


def filler(n, chrom):
    """n short intervals on a chromosome the partner does not use (chrom 2: list1's, chrom 3: list2's)."""
    return [(chrom, 100 * k, 100 * k + 10, 10) for k in range(n)]


def with_at(n, chrom, places):
    """n fillers on ``chrom`` with ``places`` = {index: interval} put in."""
    out = filler(n, chrom)
    for k, iv in places.items():
        out[k] = iv
    return out


# ---------------------------------------------------------------------------------- matching
def unsorted_data(reads, qlen2, nal):
    """The `data` list of ``reads`` read after read, NOT start-sorted: a data position is then the CSR index,
    the index is uploaded without iv_data_pos, and ties of equal (start, end) rank by CSR index."""
    from fslr_amd.prep import IntervalData
    code = np.repeat(np.arange(len(reads)), [len(r) for r in reads])
    flat = np.array([x for r in reads for x in r], np.int64).reshape(-1, 4)
    q2, na = np.asarray(qlen2, np.int64), np.asarray(nal, np.int64)
    return IntervalData(chrom=flat[:, 0], start=flat[:, 1], end=flat[:, 2], aln_size=flat[:, 3], qcode=code,
                        qnames=np.asarray([f'r{k}' for k in range(len(reads))], dtype=object),
                        n_alignments=na[code], qlen2=q2[code], middle=(flat[:, 1] + flat[:, 2]) // 2,
                        index=np.arange(flat.shape[0], dtype=np.int64))


def lists_of(data, csr):
    """Per real read rank its list of (chrom, start, end, aln_size), chromosomes in the data's own values."""
    dp = np.asarray(csr.data_pos, np.int64)
    out = []
    for r in range(csr.n_reads):
        k = dp[csr.read_off[r]:csr.read_off[r + 1]]
        out.append(list(zip(data.chrom[k].tolist(), data.start[k].tolist(), data.end[k].tolist(),
                            data.aln_size[k].tolist())))
    return out


def match_ref_any(data, csr, queries, pct, cuts, emit_mask, qd=QLEN_DIFF, nd=NAL_DIFF):
    """match_ref.match_ref for lists of any length: candidates from search_ref.brute_force reduced to first
    visits of REAL reads (match_ref.candidates), I / U from the C oracle, EDGE from Python floats."""
    import match_ref as mr
    lists = lists_of(data, csr)
    cands, _ = mr.candidates(data, csr, queries)
    rows, off, counts, best = [], [0], [], []
    for q, cs in enumerate(cands):
        ex = -1 if queries.exclude is None else int(queries.exclude[q])
        n_c = n_g = n_e = 0
        top = (-1, 0, 1)
        for p in cs.tolist():
            if p == ex:
                continue
            I, U, zd = fit(queries.reads[q], lists[p], pct)
            fl = flag_byte(I, U, zd, int(queries.qlen2[q]), int(csr.read_qlen2[p]), int(queries.nal[q]),
                           int(csr.read_nal[p]), cuts, qd, nd)
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
