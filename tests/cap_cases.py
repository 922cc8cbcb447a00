"""The hand-built inputs of the edge cap's directed tests (tests/test_cap_ref.py asserts each input's
premise from tests/cap_ref.py alone; tests/test_gpu_cap_directed.py runs them on the device).  TEST
INFRASTRUCTURE ONLY.

An input is written as named reads with their intervals; build() puts the intervals into the
reference's `data` order (a stable sort by start, cluster.py:116-121), ranks the reads by their first
appearance there (:189-191) and returns a prep.CSR with the name -> rank map.  Every case asserts the
ranks it relies on.
"""
from __future__ import annotations

import functools

import numpy as np

import cap_ref as R
from fslr_amd.prep import CSR

CUT0 = dict(R.DEFAULT, cutoffs=(0.0,))            # every counted pair is an edge
LEN = 1000                                        # interval length of the piles: shifts up to 200 still match at 0.8


class Case:
    def __init__(self, csr, rank, params, thr, note=''):
        self.csr, self.rank, self.params, self.thr, self.note = csr, rank, params, thr, note
        self.n = csr.n_reads

    @functools.cached_property
    def exp(self):
        return R.expected(self.csr, self.params, self.thr)


def build(reads, q=None, m=None, n_chroms=1):
    """reads: {name: [(start, end) | (start, end, aln) | (start, end, aln, chrom)]}, or a list of (name,
    interval), in writing order (the tie order of equal starts); q / m: {name: qlen2 / n_alignments},
    default 100 / 3."""
    q, m = q or {}, m or {}
    pairs = reads if isinstance(reads, list) else [(nm, iv) for nm, ivs in reads.items() for iv in ivs]
    flat = [(iv[0], k, name, iv) for k, (name, iv) in enumerate(pairs)]
    flat.sort(key=lambda t: (t[0], t[1]))                   # stable by start
    rank, per = {}, {}
    for pos, (_, _, name, iv) in enumerate(flat):
        rank.setdefault(name, len(rank))
        per.setdefault(name, []).append((pos, iv))
    names = list(rank)
    off, cols = [0], {k: [] for k in ('chrom', 'start', 'end', 'aln', 'dp')}
    for name in names:
        for pos, iv in per[name]:
            cols['start'].append(iv[0])
            cols['end'].append(iv[1])
            cols['aln'].append(iv[2] if len(iv) > 2 and iv[2] is not None else iv[1] - iv[0])
            cols['chrom'].append(iv[3] if len(iv) > 3 else 0)
            cols['dp'].append(pos)
        off.append(len(cols['start']))
    assert max(np.diff(off)) <= 64
    n = len(names)
    csr = CSR(read_off=np.array(off, np.int32), read_qlen2=np.array([q.get(x, 100) for x in names], np.int32),
              read_nal=np.array([m.get(x, 3) for x in names], np.int32), iv_chrom=np.array(cols['chrom'], np.int32),
              iv_start=np.array(cols['start'], np.int32), iv_end=np.array(cols['end'], np.int32),
              iv_aln=np.array(cols['aln'], np.int64), n_chroms=n_chroms, read_qcode=np.arange(n, dtype=np.int64),
              data_pos=np.array(cols['dp'], np.int64), nal_varies=False)
    return csr, rank


def iv(start, length=LEN, aln=None):
    return (start, start + length, aln)


# ------------------------------------------------------------------------------------ A: closure graphs
def ladder(depth, thr=3):
    """Read 0 is the only seed (thr + 1 forward rows); rung k = read k has thr - 1 forward rows, one of
    them to rung k + 1, so it joins in round k through rung k - 1 alone.  The other rows end in sinks
    (reads above the rungs, one back count each).  Returns (n, rows)."""
    rows, sink = [], depth + 1
    rows.append((0, 1))
    for _ in range(thr):
        rows.append((0, sink))
        sink += 1
    for k in range(1, depth + 1):
        if k < depth:
            rows.append((k, k + 1))
        for _ in range(thr - 1 - (k < depth)):
            rows.append((k, sink))
            sink += 1
    return sink, rows


def fan(width=129, thr=2):
    """A seed whose `width` forward rows each complete one join: target i has thr - 1 rows to sinks of
    its own."""
    rows = [(0, 1 + i) for i in range(width)] + [(0, 1 + width)]          # width + 1 > thr rows
    sink = 2 + width
    for i in range(width):
        for _ in range(thr - 1):
            rows.append((1 + i, sink))
            sink += 1
    return sink, rows


def two_rounds():
    """thr = 2.  Read 0 is a seed; read 1 joins in round 1 (one forward row, one back count); read 5 has
    no forward row and back counts from read 0 (round 0) and read 1 (round 1): it joins in round 2."""
    return 8, [(0, 1), (0, 5), (0, 6), (1, 5), (2, 7)]


def only_seeds():
    """thr = 3: reads 0 and 4 are seeds; nobody they point at reaches 3."""
    return 12, [(0, 1), (0, 2), (0, 3), (0, 8), (4, 5), (4, 6), (4, 7), (4, 8), (1, 9), (5, 9)]


def everyone(n=70):
    """thr = 1: a chain with chords; the last read has no forward row and joins by its back count."""
    return n, [(k, k + 1) for k in range(n - 1)] + [(k, k + 5) for k in range(0, n - 5, 3)]


def closure_shapes():
    out = {f'ladder{d}': (3,) + ladder(d) for d in (7, 8, 9, 15, 16, 17, 31, 32, 33, 40)}
    out['fan129'] = (2,) + fan()
    out['two_rounds'] = (2,) + two_rounds()
    out['only_seeds'] = (3,) + only_seeds()
    out['everyone'] = (1,) + everyone()
    return out


def ordered(rows, order):
    rows = sorted(rows)
    if order == 'reversed':
        return rows[::-1]
    if order == 'shuffled':
        return [rows[k] for k in np.random.default_rng(5).permutation(len(rows))]
    return rows


def witness_reads(n):
    """Graph read x (rank 2x) has one interval on a locus it shares with its witness (rank 2x + 1) alone."""
    reads = {}
    for x in range(n):
        reads[f'g{x}'] = [iv(10_000 * x)]
        reads[f'w{x}'] = [iv(10_000 * x + 10)]
    csr, rank = build(reads)
    assert all(rank[f'g{x}'] == 2 * x and rank[f'w{x}'] == 2 * x + 1 for x in range(n))
    return csr


# ------------------------------------------------------------------------------------ B: visit lists
def tie_run(count, ends):
    """One T read `x` (two intervals) and a run of `count` single-interval reads of equal start inside its
    first interval's hits, between `above` reads of higher and `below` reads of lower distinct starts.
    ends: 'distinct' | 'equal' | 'mixed'.  x's second interval has the run's start too (it is dropped from
    its own list without shifting the ranks).  Also: a read whose end is exactly x's start (a hit) next to
    one that ends one before it (none); every pile read matches every other (cut 0: edges), thr = 2."""
    S = 50_000
    reads = [('x', iv(S))]
    reads.append(('touch', (S - 900, S, None)))            # end == start_x: inside
    reads.append(('miss', (S - 901, S - 1, None)))         # end == start_x - 1: outside
    for k in range(7):
        reads.append((f'lo{k}', iv(S + 1 + k, LEN + k % 3)))
    run_start = S + 20
    for k in range(count):
        e = {'distinct': LEN + k, 'equal': LEN, 'mixed': LEN + (k % 4) * 3}[ends]
        reads.append((f't{k}', iv(run_start, e)))
        if k == count // 2:
            reads.append(('x', iv(run_start, LEN + 1)))
    for k in range(9):
        reads.append((f'hi{k}', iv(S + 30 + k, LEN - k % 2)))
    csr, rank = build(reads)
    return Case(csr, rank, CUT0, 2)


def directions():
    """A T read `x` with an interval whose hits are all backward (lower positions), one whose hits are
    all forward, and one with none; reads `p` and `q` are both in T and share a start (k_cap_tq_bs scans
    the equal-start run for its own record).  thr = 2, cut 0."""
    reads = {'b0': [iv(1000)], 'b1': [iv(1001)], 'b2': [iv(1002)],
             'x': [iv(1003), iv(20_000), iv(40_000)],
             'f0': [iv(20_001)], 'f1': [iv(20_002)], 'f2': [iv(20_003)],
             'p': [iv(60_000), iv(60_500)], 'q': [iv(60_000), iv(60_501)],
             'r0': [iv(60_001)], 'r1': [iv(60_002)], 'r2': [iv(60_003)]}
    csr, rank = build(reads)
    return Case(csr, rank, CUT0, 2)


# ------------------------------------------------------------------------------------ C: loops
def one_locus(thr, n=200):
    """n single-interval reads, read r at start 5000 + r: every pair matches (I = U = 1, an edge under the
    default cuts).  Read 0's list is n - 1, ..., 1, all new edges: its first break is at list index thr - 1."""
    csr, rank = build({f'r{r}': [iv(5000 + r)] for r in range(n)})
    assert all(rank[f'r{r}'] == r for r in range(n))
    return Case(csr, rank, R.DEFAULT, thr)


LOCI = (100_000, 200_000, 300_000, 400_000)
FILLER = dict(q=1000, m=30)                        # fails both ratios of the gate against q = 100, m = 3


def walks(k, kind, thr=3):
    """x has four intervals (loci A, B, C, D); `thr` twins w1.. have the same four and v has A, B and D
    below them (thr + 1 forward edges: the cap binds), so x's loop breaks in A at list index thr - 1.  B lists k fillers (higher starts; the length gate fails against x and the twins;
    aln so large that they match nothing) and then z: kind 'edge': z has B, C, D (I = 3, U = 4 with x);
    'counted': z has B and two private intervals (I = 1 of L = 3: counted, below the cut).  C lists only
    reads x has seen (the walk runs off the end); D lists one filler and z2, a single interval (counted)."""
    A, B, C, D = LOCI
    reads = {'x': [iv(A), iv(B), iv(C), iv(D)]}
    reads['v'] = [iv(A + 1), iv(B + 1), iv(D + 1)]            # one more partner than the cap: left behind in A
    for j in range(1, thr + 1):
        reads[f'w{j}'] = [iv(A + 1 + j), iv(B + 1 + j), iv(C + 1 + j), iv(D + 1 + j)]
    if kind == 'edge':
        reads['z'] = [iv(B + 50), iv(C + 50), iv(D + 50)]
    else:
        reads['z'] = [iv(B + 50), iv(250_000), iv(260_000)]
    q, m = {}, {}
    for f in range(k):
        reads[f'f{f}'] = [iv(B + 100 + f, LEN, 10 ** 7)]
    reads['g0'] = [iv(D + 100, LEN, 10 ** 7)]
    reads['z2'] = [iv(D + 60)]
    for name in reads:
        if name[0] in 'fg':
            q[name], m[name] = FILLER['q'], FILLER['m']
    csr, rank = build(reads, q, m)
    assert rank['x'] == 0
    return Case(csr, rank, R.DEFAULT, thr)


def empty_segments(thr=3):
    """x: a private interval (no hit), the pile A (the break), a private one, the pile B (a walk), a
    private one.  The twins have the same shape, so the last read of T ends in an empty segment too."""
    A, B = 100_000, 200_000
    reads = {}
    for j, name in enumerate(['x'] + [f'w{k}' for k in range(1, thr + 2)]):
        reads[name] = [iv(10_000 + 2000 * j), iv(A + j), iv(150_000 + 2000 * j), iv(B + j), iv(300_000 + 2000 * j)]
    reads['z'] = [iv(B + 50), iv(320_000)]
    csr, rank = build(reads)
    assert rank['x'] == 0
    return Case(csr, rank, CUT0, thr)


def eval_mix(thr=5):
    """24 reads of 1, 16, 17 and 64 intervals stacked on one locus (starts 5000 + U[0, 300], lengths 1000 +
    U[0, 300]): every pair is counted, the cut-0 table makes each an edge, the cap binds."""
    rng = np.random.default_rng(17)
    Ls = [1, 16, 17, 64, 17, 16, 16, 17] * 3
    reads = {}
    for r, L in enumerate(Ls):
        st = np.sort(5000 + rng.integers(0, 301, L))
        reads[f'r{r}'] = [iv(int(s), int(1000 + rng.integers(0, 301))) for s in st]
    csr, rank = build(reads)
    return Case(csr, rank, CUT0, thr)


def left_behind():
    """thr = 2, cut 0.  y's loop (A: p1, p2 first) breaks before x and x2.  x fails the gate against p1 and
    p2, so its own loop reaches y: (y, x) appears as (x, y).  x2's loop breaks on p1, p2: (y, x2) is left by
    both loops and dropped.  u (lowest rank, one forward edge: outside T) shares locus B with y: (u, y) is
    formed in u's loop and stays (u, y)."""
    A, B = 100_000, 200_000
    reads = {'u': [iv(1000), iv(B)], 'y': [iv(A), iv(B + 1)], 'x': [iv(A + 1)], 'x2': [iv(A + 2)],
             'p2': [iv(A + 10)], 'p1': [iv(A + 11)]}
    q = {'y': 100, 'p1': 104, 'p2': 104, 'x': 97, 'x2': 100, 'u': 100}
    m = {'y': 4, 'p1': 5, 'p2': 5, 'x': 3, 'x2': 4, 'u': 4}
    csr, rank = build(reads, q, m)
    assert [rank[k] for k in ('u', 'y', 'x', 'x2', 'p2', 'p1')] == [0, 1, 2, 3, 4, 5]
    return Case(csr, rank, CUT0, 2)


def hole_fill(where, pile=30, thr=3):
    """A pile of `pile` mutually matching reads (T) and `few` matching pairs that the cap leaves alone, the
    pile at the 'end' or the 'start' of the rank order (the sweep's edge list: one run per read in rank
    order); 'start' leaves fewer surviving tail rows (3) than the pile's dropped rows."""
    lo, hi = (10_000, 500_000) if where == 'start' else (500_000, 10_000)
    reads = {f'r{r}': [iv(lo + r)] for r in range(pile)}
    for k in range(3 if where == 'start' else 12):
        reads[f'a{k}'] = [iv(hi + 5000 * k)]
        reads[f'b{k}'] = [iv(hi + 5000 * k + 1)]
    csr, rank = build(reads)
    return Case(csr, rank, R.DEFAULT, thr)


def threshold_zero(thr):
    """60 reads: a pile of 20 (two intervals each, so later intervals walk), 10 matching pairs, 10 pairs that
    are counted but no edge (one shared locus of three), and 20 reads with no hit at all."""
    reads = {}
    for r in range(20):
        reads[f'r{r}'] = [iv(5000 + r), iv(50_000 + (7 * r) % 20)]
    for k in range(5):
        reads[f'a{k}'] = [iv(100_000 + 5000 * k)]
        reads[f'b{k}'] = [iv(100_000 + 5000 * k + 1)]
    for k in range(5):
        base = 200_000 + 20_000 * k
        reads[f'c{k}'] = [iv(base), iv(base + 3000), iv(base + 6000)]
        reads[f'd{k}'] = [iv(base + 1), iv(base + 9000), iv(base + 12_000)]
    for k in range(20):
        reads[f'e{k}'] = [iv(400_000 + 5000 * k)]
    csr, rank = build(reads)
    assert csr.n_reads == 60
    return Case(csr, rank, R.DEFAULT, thr)


BREAK_THR = (1, 2, 63, 64, 65, 128, 129)
FILLERS = (0, 62, 63, 64, 65, 128)
TIE_COUNTS = (63, 64, 65, 130)
TIE_ENDS = ('distinct', 'equal', 'mixed')


@functools.lru_cache(maxsize=None)
def case(name, *args):
    return globals()[name](*args)


def loop_cases():
    """(id, builder, args) of every section-C input."""
    out = [(f'break{t}', 'one_locus', (t,)) for t in BREAK_THR]
    out += [(f'walk{k}_{kind}', 'walks', (k, kind)) for k in FILLERS for kind in ('edge', 'counted')]
    out += [('empty_segments', 'empty_segments', ()), ('eval_mix', 'eval_mix', ()), ('left_behind', 'left_behind', ()),
            ('holes_end', 'hole_fill', ('end',)), ('holes_start', 'hole_fill', ('start',)),
            ('thr0', 'threshold_zero', (0,)), ('thr-1', 'threshold_zero', (-1,))]
    return out


def list_cases():
    out = [(f'tie{c}_{e}', 'tie_run', (c, e)) for c in TIE_COUNTS for e in TIE_ENDS]
    return out + [('directions', 'directions', ())]
