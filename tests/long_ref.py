"""Plain reference for the graph of reads of any length, and the directed inputs of the long-read tests
(reads of more than 64 intervals: chunk seams, the 4096 limit, dense blocks, rank orders).  Test
infrastructure only; not a test module.

The reference restates the reference program's pair loop without its edge cap: calculate_overlap
(cluster.py:133-136), overall_jaccard_similarity (:140-170), different_lengths_or_alignments (:178-183) and
the loop around them (:197-222), over whole interval lists and with Python floats.  It is written from those
lines, not from the device kernels, their host emulation or the C oracle; tests/test_long_ref.py holds it
against the C oracle on every input below.

A read's list is its intervals in `data` order (start ascending, ties in the given order); reads rank by
their first appearance there, and the pair loop meets a pair first in its lower-rank read's loop, so list1 is
the lower-rank read's list.
"""
import functools

import numpy as np

from match_ref import resident_data
from pairs_ref import union_find_labels

CUTS = [1, 1, 0.66, 0.66, 0.66, 0.5]
QLEN_DIFF, NAL_DIFF = 0.04, 0.25
MAX_READ = 4096                              # the device's limit on a read's intervals
QLEN2, NAL = 1000, 4                         # what every read gets unless an input says otherwise


# ---------------------------------------------------------------------------------- the reference
def calculate_overlap(x, y):
    """cluster.py:133-136 for intervals (chrom, start, end, aln_size)."""
    shared = max(0, min(x[2], y[2]) - max(x[1], y[1]))
    return min(shared / x[3], shared / y[3])


def lengths_differ(q1, q2, n1, n2, qlen_diff, diff):
    """cluster.py:178-183."""
    if min(q1, q2) / max(q1, q2) >= 1 - qlen_diff:
        return False
    if min(n1, n2) / max(n1, n2) >= 1 - diff:
        return False
    return True


def first_fit(l1, l2, overlap):
    """I of cluster.py:152-161: rows of l1 in order, each takes the lowest column of l2 that no earlier row
    took, lies on its chromosome and has calculate_overlap >= overlap.  Only a row's own chromosome's columns
    are visited (the others fail :157's first test), and the taken columns at the front of a chromosome's
    list are stepped over once (:155 skips them for every later row)."""
    cols = {}
    for j, y in enumerate(l2):
        cols.setdefault(y[0], []).append(j)
    front = dict.fromkeys(cols, 0)
    taken = [False] * len(l2)
    n_i = 0
    for x in l1:
        mine = cols.get(x[0])
        if mine is None:
            continue
        h = front[x[0]]
        while h < len(mine) and taken[mine[h]]:
            h += 1
        front[x[0]] = h
        for t in range(h, len(mine)):
            j = mine[t]
            if taken[j]:
                continue
            if calculate_overlap(x, l2[j]) >= overlap:
                taken[j] = True
                n_i += 1
                break
    return n_i


def matching_cells(l1, l2, overlap):
    """Every (row, column) that :157 accepts, whatever was taken."""
    return [(i, j) for i, x in enumerate(l1) for j, y in enumerate(l2)
            if x[0] == y[0] and calculate_overlap(x, y) >= overlap]


def first_fit_cells(cells):
    """first_fit over a cell list (rows ascending, the lowest free column)."""
    rows = {}
    for i, j in cells:
        rows.setdefault(i, []).append(j)
    taken = set()
    for i in sorted(rows):
        for j in sorted(rows[i]):
            if j not in taken:
                taken.add(j)
                break
    return len(taken)


def max_matching(cells):
    """The size of a maximum matching of the cells (augmenting paths)."""
    rows = {}
    for i, j in cells:
        rows.setdefault(i, []).append(j)
    row_of = {}

    def augment(i, seen):
        for j in rows[i]:
            if j in seen:
                continue
            seen.add(j)
            if j not in row_of or augment(row_of[j], seen):
                row_of[j] = i
                return True
        return False
    return sum(augment(i, set()) for i in rows)


def lists_touch(l1, l2):
    """Does the pair loop meet this pair at all (cluster.py:199-208): some interval of one read is a search
    hit of an interval of the other, that is same chromosome, s1 <= e2 and e1 >= s2.  One pass in (chrom,
    start) order, keeping how far each read's intervals seen so far reach."""
    events = sorted([(x[0], x[1], 0, x[2]) for x in l1] + [(y[0], y[1], 1, y[2]) for y in l2])
    reach = {}
    for chrom, start, side, end in events:
        if reach.get((chrom, 1 - side), -1) >= start:
            return True
        reach[(chrom, side)] = max(reach.get((chrom, side), -1), end)
    return False


def read_lists(csr):
    """Per read rank its list of (chrom, start, end, aln_size)."""
    off = np.asarray(csr.read_off).tolist()
    flat = list(zip(np.asarray(csr.iv_chrom).tolist(), np.asarray(csr.iv_start).tolist(),
                    np.asarray(csr.iv_end).tolist(), np.asarray(csr.iv_aln).tolist()))
    return [flat[off[r]:off[r + 1]] for r in range(len(off) - 1)]


def pair_scores(csr, overlap, qlen_diff=QLEN_DIFF, diff=NAL_DIFF):
    """[(a, b, I, U)], a < b read ranks, of every pair the loop evaluates: met (lists_touch) and through the
    length gate.  I may be 0."""
    lists = read_lists(csr)
    chroms = [set(x[0] for x in l) for l in lists]
    q, m = np.asarray(csr.read_qlen2).tolist(), np.asarray(csr.read_nal).tolist()
    out = []
    for a in range(len(lists)):
        for b in range(a + 1, len(lists)):
            if not chroms[a] & chroms[b] or not lists_touch(lists[a], lists[b]):
                continue
            if lengths_differ(q[a], q[b], m[a], m[b], qlen_diff, diff):
                continue
            n_i = first_fit(lists[a], lists[b], overlap)
            out.append((a, b, n_i, len(lists[a]) + len(lists[b]) - n_i))
    return out


class Graph:
    """edges: the sorted [(a, b, I, U)]; fwd[a]: a's edges as the lower rank; labels[r]: the smallest rank of
    r's component; comp[r]: the component's number among those of two or more reads, by smallest rank
    (-1: r has no edge)."""

    def __init__(self, n, edges):
        self.n, self.edges = n, sorted(edges)
        self.fwd = np.bincount([e[0] for e in edges], minlength=n).astype(np.int64)
        self.labels = union_find_labels(n, edges)
        sizes = np.bincount(self.labels, minlength=n)
        number = np.full(n, -1, np.int64)
        number[np.flatnonzero(sizes >= 2)] = np.arange(int((sizes >= 2).sum()))
        self.comp = np.where(sizes[self.labels] >= 2, number[self.labels], -1)


def graph_of(n, scores, cutoffs):
    """cluster.py:216-221 over pair_scores' list."""
    cut = [float(c) for c in cutoffs]
    edges = []
    for a, b, n_i, union in scores:
        if n_i == 0:
            continue
        target = cut[n_i - 1] if n_i - 1 < len(cut) else cut[-1]
        if n_i / union >= target:
            edges.append((a, b, n_i, union))
    return Graph(n, edges)


def long_ref(csr, overlap, cutoffs, qlen_diff=QLEN_DIFF, diff=NAL_DIFF):
    """The uncapped graph of a rank-ordered CSR (what ``data.csr()`` gives)."""
    return graph_of(csr.n_reads, pair_scores(csr, overlap, qlen_diff, diff), cutoffs)


# ---------------------------------------------------------------------------------- builders
def reads_to_data(reads, qlen2=None, nal=None):
    """The `data` list of ``reads`` (per read a list of (chrom, start, end, aln_size)): start ascending, ties
    in the given order (read after read), so of two reads that begin at one start the earlier listed ranks
    lower.  Read k is 'r<k>'."""
    qlen2 = [QLEN2] * len(reads) if qlen2 is None else qlen2
    nal = [NAL] * len(reads) if nal is None else nal
    return resident_data(reads, qlen2, nal)


def rank_of(data):
    """{k: the rank of read 'r<k>'}."""
    names = data.qnames[data.csr().read_qcode].tolist()
    return {int(name[1:]): r for r, name in enumerate(names)}


def oracle_from_csr(c):
    from oracle import oracle as O
    cnt = np.diff(c.read_off)
    return O.OracleCSR(c.read_off, c.iv_chrom, c.iv_start, c.iv_end, c.iv_aln, np.repeat(c.read_qlen2, cnt),
                       np.repeat(c.read_nal, cnt), c.data_pos)


def bystanders():
    """Three short reads on a chromosome of their own: the first two hold the same three intervals (an edge
    at every cutoff list used here), the third shares one of them (I = 1 of U = 5: no edge)."""
    iv = [(9, 5_000_000 + 2000 * k, 5_000_500 + 2000 * k, 500) for k in range(3)]
    return [list(iv), list(iv), [iv[1], (9, 5_100_000, 5_100_500, 500), (9, 5_200_000, 5_200_500, 500)]]


# ---------------------------------------------------------------------------------- the directed inputs
def diagonal(la, lb):
    """Interval k of both reads at k * 10_000 on one chromosome: cell (k, k) matches and nothing else, so
    I = min(la, lb).  Read 0 (la intervals) ranks below read 1."""
    row = lambda k: (1, 10_000 * k, 10_000 * k + 1000, 1000)
    return reads_to_data([[row(k) for k in range(la)], [row(k) for k in range(lb)]] + bystanders())


def last_chunk(kind):
    """Two reads of 4096 intervals whose only matches lie at the far end of the lists.
    'tail': rows 4033..4095 against columns 4033..4095 (cell (k, k) at a positive overlap, the whole 63 x 63
    block at overlap <= 0); 'row0': row 0 x column 4095 alone; 'col0': row 4095 x column 0 alone.
    Every other interval lies on a chromosome only its own read uses."""
    n = MAX_READ
    if kind == 'tail':
        a = [(2, 100 * k, 100 * k + 10, 10) for k in range(n - 63)]
        b = [(3, 100 * k, 100 * k + 10, 10) for k in range(n - 63)]
        shared = [(1, 1_000_000 + 10_000 * k, 1_001_000 + 10_000 * k, 1000) for k in range(63)]
        return reads_to_data([a + shared, b + shared] + bystanders())
    if kind == 'row0':
        # row 0 must start no later than every column and still reach the last one: a long span whose
        # aln_size (a column of its own in the input) is the last column's
        a = [(1, 0, 451_000, 1000)] + [(2, 1_000_000 + 100 * k, 1_000_010 + 100 * k, 10) for k in range(n - 1)]
        b = [(3, 100 + 100 * k, 110 + 100 * k, 10) for k in range(n - 1)] + [(1, 450_000, 451_000, 1000)]
        return reads_to_data([a, b] + bystanders())
    if kind == 'col0':
        a = [(2, 100 * k, 100 * k + 10, 10) for k in range(n - 1)] + [(1, 1_000_000, 1_001_000, 1000)]
        b = [(1, 1_000_000, 1_001_000, 1000)] + [(3, 2_000_000 + 100 * k, 2_000_010 + 100 * k, 10) for k in range(n - 1)]
        return reads_to_data([a, b] + bystanders())
    raise ValueError(kind)


def full_block(lens, qlen2=None, nal=None):
    """Every interval of every read is (1, 1000, 2000): every row matches every column, a read's own chunks
    overlap each other, I = min(L) and U = max(L) for every pair.  Ranks follow the order of ``lens``."""
    n_by = len(bystanders())
    qlen2 = None if qlen2 is None else list(qlen2) + [QLEN2] * n_by
    nal = None if nal is None else list(nal) + [NAL] * n_by
    return reads_to_data([[(1, 1000, 2000, 1000)] * L for L in lens] + bystanders(), qlen2, nal)


def gadgets(la, lb, places, swap=False):
    """Two reads A (la intervals) and B (lb) with, per (r0, r1, c0, c1) of ``places`` (ascending, disjoint),
    A's intervals r0 < r1 and B's intervals c0 < c1 such that r0 matches {c0, c1} and r1 matches {c0} alone at
    overlap 0.5: first-fit gives the gadget 1 (r0 takes c0) where a maximum matching has 2, and the same with
    the lists exchanged (c0 matches {r0, r1}, c1 matches {r0}).  The gadgets lie 10_000_000 apart on
    chromosome 1.  The other intervals: identical isolated intervals on chromosome 4 in both reads (the k-th of
    A matches the k-th of B), as many as fit in front of each gadget and behind the last, and short intervals
    on chromosomes 2 (A) and 3 (B) that match nothing where one read needs more in front of a gadget, or
    between its two gadget intervals, than the other.  Those in front start where r0 and c0 start, listed
    before them, so both reads always begin at one start: the read listed first, A unless ``swap``, ranks
    lower and is list1."""
    A, B = [], []
    for g, (r0, r1, c0, c1) in enumerate(places):
        base = 10_000_000 * (g + 1)
        na, nb = r0 - len(A), c0 - len(B)
        assert na >= 0 and nb >= 0, places
        both = min(na, nb)
        fill = [(4, base - 2_000_000 + 1000 * k, base - 2_000_000 + 1000 * k + 500, 500) for k in range(both)]
        A += fill + [(2, base, base + 2, 2)] * (na - both)
        B += fill + [(3, base, base + 2, 2)] * (nb - both)
        assert r1 - r0 - 1 < 300 and c1 - c0 - 1 < 500
        A += [(1, base, base + 140_000, 140_000)]
        A += [(2, base + 10 + 100 * k, base + 20 + 100 * k, 10) for k in range(r1 - r0 - 1)]
        A += [(1, base + 36_000, base + 96_000, 60_000)]
        B += [(1, base, base + 100_000, 100_000)]
        B += [(3, base + 2000 + 100 * k, base + 2010 + 100 * k, 10) for k in range(c1 - c0 - 1)]
        B += [(1, base + 60_000, base + 160_000, 100_000)]
    base = 10_000_000 * (len(places) + 1)
    na, nb = la - len(A), lb - len(B)
    assert na >= 0 and nb >= 0
    both = min(na, nb)
    fill = [(4, base + 1000 * k, base + 1000 * k + 500, 500) for k in range(both)]
    A += fill + [(2, base + 3_000_000 + 100 * k, base + 3_000_010 + 100 * k, 10) for k in range(na - both)]
    B += fill + [(3, base + 3_500_000 + 100 * k, base + 3_500_010 + 100 * k, 10) for k in range(nb - both)]
    return reads_to_data(([B, A] if swap else [A, B]) + bystanders())


def _more(first, n=9):
    """n further gadget places of two adjacent rows and columns each, from index ``first`` = (row, column)."""
    return [(first[0] + 5 * t, first[0] + 5 * t + 1, first[1] + 5 * t, first[1] + 5 * t + 1) for t in range(n)]


GADGET_PLACES = {                 # the seam gadget and nine more (five in the short read): I = maximum - gadgets
    'g63_64x63_64': (100, 100, _more((1, 1)) + [(63, 64, 63, 64)]),
    'g0_64x63_64': (130, 130, [(0, 64, 63, 64)] + _more((66, 66))),
    'g63_64x0_127': (130, 200, [(63, 64, 0, 127)] + _more((66, 129))),
    'g127_128x64_128': (130, 130, _more((1, 1)) + [(127, 128, 64, 128)]),
    'g63_64x38_39_short': (100, 40, _more((1, 12), 5) + [(63, 64, 38, 39)]),   # a long read against a short one
}


def gate(qn):
    """full_block of lengths 130, 130, 70 with ``qn`` = the three reads' (qlen2, n_alignments)."""
    return full_block([130, 130, 70], [x[0] for x in qn], [x[1] for x in qn])


GATES = {
    # different_lengths_or_alignments at qlen_diff 0.04, diff 0.25: r0-r1 fail both ratios (0.5, 0.5) though
    # every chunk pair matches; r2 passes against r0 (equal) and fails against r1
    'gate_fail': [(1000, 10), (500, 5), (1000, 10)],
    # at equality: 96 / 100 >= 1 - 0.04 passes on qlen2 alone (n_alignments 2 / 4 fails); r2 passes r0 on
    # n_alignments alone, 3 / 4 >= 1 - 0.25, its qlen2 95 / 100 fails; r1-r2: 95 / 96 passes
    'gate_equal': [(100, 4), (96, 2), (95, 3)],
    # one below equality on both: r0-r1 95 / 100 and 2 / 4 fail; r0-r2 fails 94 / 100 and 2 / 4;
    # r1-r2 passes (94 / 95)
    'gate_below': [(100, 4), (95, 2), (94, 2)],
}


def many_chromosomes():
    """Read 0: 200 intervals alternating over chromosomes 1, 2, 3; read 1: 200 of the same interval as 60 of
    chromosome 1, then 67 of 2, then 73 of 3.  All intervals are (chrom, 1000, 2000), so a list's order is the
    order given and chunk membership cuts across chromosome membership: I = 60 + 67 + 66 = 193, U = 207."""
    a = [(1 + k % 3, 1000, 2000, 1000) for k in range(200)]
    b = [(1, 1000, 2000, 1000)] * 60 + [(2, 1000, 2000, 1000)] * 67 + [(3, 1000, 2000, 1000)] * 73
    return reads_to_data([a, b] + bystanders())


class Case:
    """One directed input: ``data()`` builds it (once), ``overlap`` is the positive overlap cutoff it is made
    for, ``cuts`` the two cutoff lists it runs with, ``max_len`` the longest read it must hold, ``pair`` =
    (I, U) expected of reads r0 / r1 whenever they form an edge (None: the reference alone says),
    ``gadget`` = the input must have first_fit < max_matching for r0 / r1 at ``overlap``."""

    def __init__(self, name, build, max_len, overlap=0.8, cuts=(CUTS, [0.5]), pair=None, gadget=False):
        self.name, self._build, self.max_len, self.overlap = name, build, max_len, overlap
        self.cuts, self.pair, self.gadget = [list(c) for c in cuts], pair, gadget
        self._data, self._scores = None, {}

    def __repr__(self):
        return self.name

    def data(self):
        if self._data is None:
            self._data = self._build()
        return self._data

    def ref(self, overlap, cutoffs, qlen_diff=QLEN_DIFF, diff=NAL_DIFF):
        """long_ref of the input; the pair scores of an overlap are computed once."""
        csr = self.data().csr()
        key = (overlap, qlen_diff, diff)
        if key not in self._scores:
            self._scores[key] = pair_scores(csr, overlap, qlen_diff, diff)
        return graph_of(csr.n_reads, self._scores[key], cutoffs)


def _cases():
    out = []
    # [0.5]: an edge where I / U >= 0.5, so (65, 129) is one and (64, 129), (1, 65), (65, 1) are not
    for la, lb in [(65, 65), (64, 65), (65, 64), (128, 128), (129, 128), (128, 129), (1, 65), (65, 1), (65, 129),
                   (64, 129), (4095, 4096), (4096, 4096)]:
        out.append(Case(f'diag_{la}_{lb}', functools.partial(diagonal, la, lb), max(la, lb),
                        pair=(min(la, lb), max(la, lb))))
    # the cutoff that I / U meets exactly: one match fewer and the edge is gone; [0.5] gives no edge
    out.append(Case('last_tail', functools.partial(last_chunk, 'tail'), 4096, cuts=([63 / 8129], [0.5]),
                    pair=(63, 8129)))
    out.append(Case('last_row0', functools.partial(last_chunk, 'row0'), 4096, cuts=([1 / 8191], [0.5]),
                    pair=(1, 8191)))
    out.append(Case('last_col0', functools.partial(last_chunk, 'col0'), 4096, cuts=([1 / 8191], [0.5]),
                    pair=(1, 8191)))
    for lens in [(65, 65), (130, 130), (64, 130), (130, 64), (129, 257), (257, 129), (130, 130, 64), (64, 130, 130),
                 (130, 64, 130)]:
        # [0.3]: 64 / 130 is an edge; CUTS end at 0.5, where it is none and 129 / 257 still is one
        out.append(Case('block_' + '_'.join(map(str, lens)), functools.partial(full_block, lens), max(lens),
                        cuts=(CUTS, [0.3]), pair=(min(lens[:2]), max(lens[:2]))))
    for name, (la, lb, places) in GADGET_PLACES.items():
        for swap in (False, True):
            out.append(Case(name + ('_swapped' if swap else ''), functools.partial(gadgets, la, lb, places, swap),
                            max(la, lb), overlap=0.5, cuts=([0.05], [0.95]), gadget=True))
    for name, qn in GATES.items():
        out.append(Case(name, functools.partial(gate, qn), 130))
    out.append(Case('many_chromosomes', many_chromosomes, 200, pair=(193, 207)))
    return out


CASES = _cases()
CASE = {c.name: c for c in CASES}
